"""GPU: the weight-gradient stage (csrc/dw.hip) alone -- split-K GEMMs in the three arithmetics, slab and tile-partial reductions,
weight-norm fold -- on operand tiles the test writes itself into a workspace carved as tests/dw_util.py restates it.

No chain kernel runs here: the operands of this stage are plain saved tiles, so every case
  1. carves one allocation for its point count, 2. writes synthetic operand tiles, tile partials and (SPLIT_F16) the absmax / tmax
  words and the arithmetic tag computed from those tiles, 3. fills the slabs, the reduced block, tred and the gradient with NaN,
  4. calls dh_weight_grads_gemm_ex and dh_weight_grads_fold, 5. checks that every workspace region other than slabs and tred
  (gesave behind the slabs included) is bitwise what it wrote.

(a) EXACT.  Operands are independent uniform integers in [-8, 8]; ntiles sweeps 1..40 and {63, 64, 65, 255, 256, 257}: below, at and
    above a job group's workgroup count, the 64-way tile-partial split and DW_G = 256, so workgroups that own no tile, one tile or
    an uneven share all occur.  Every job's reduced slab must EQUAL the int64 product, in all three arithmetics.  Why equality is
    owed: |x| <= 8 is one bf16 piece (the other two pieces are zero) and one fp32 value; in the two-piece fp16 form the scales are
    powers of two read from the words the test writes (maximum 8 -> S = 2^5, the embedding's constant 16), so a scaled operand is an
    integer multiple of 16 below 2^9 -- one fp16 value, zero residual -- and every product, partial sum and the change-over ratio
    of a two-pair job is a power of two times an integer below 64 * 64 * 257 * 2 < 2^24: exact in the fp32 accumulators, the
    slab reduction and the division by the scale product.  The tile-partial reduction is checked the same way (integers).
(b) PRECISION.  Tame operands O(1) normal, heavy-tailed ones normal x 2^U(-20, 0) per tile, one heavy tile per class entirely zero
    (a ray that misses the object).  Per job: relative Frobenius error against the fp64 product of the same fp32 operands, bounded
    by K x the same error of torch's fp32 A^T B (TF32 off) and by 2e-4 (the whole end-to-end budget of
    tests/test_gpu_render_backward.py).  Measured on the MI355X, worst job, ntiles 3 / 65 (ratio = error / yardstick):
        split_f16   0.922 / 0.223   (errors 1.1e-7 .. 2.2e-7; torch fp32 1.4e-7 .. 2.5e-7 at 3 tiles, 0.9e-6 .. 1.3e-6 at 65)
        split_bf16  1.099 / 0.253
        fp32_mfma   1.334 / 0.382
    K = 2 x the larger ratio (seeds and boxes are all that vary): 1.844, 2.198, 2.668.
(c) FOLD.  Real parameters, case (a)'s integers at ntiles 1 and 33: the flat gradient against dw_util.fold_reference (fp64, autograd
    through W = g v / |v|), per parameter tensor by maximum error relative to the tensor's maximum, bounded by K_FOLD x the same
    figure of fold_reference evaluated in fp32.  Measured worst ratio 1.613 at 1 tile, 2.567 at 33 (colour
    lin4.weight_v, whose fp32 reference happens to be good to 5.8e-8; the slabs are exact, so the three arithmetics agree);
    K_FOLD = 2 x 2.567.  lin3 has 217 rows, the
    variance slot stays NaN, nothing else is NaN.
(d) is step 5 above, in every case, and once more on float garbage.
(e) SPLIT_F16 without the arithmetic tag, or with a non-finite class maximum, writes NaN slabs.
"""
import pytest
import torch

from tests import dw_util as U
from tests.util import flat_from_oracle, randomized_models

pytestmark = pytest.mark.gpu

ARITHS = {"split_f16": 2, "split_bf16": 0, "fp32_mfma": 1}
NT_SWEEP = list(range(1, 41)) + [63, 64, 65, 255, 256, 257]
NT_MAX = max(NT_SWEEP)
INT_REGIONS = U.OPERAND_REGIONS + ("rsave",)

# measured ratios (module docstring) x 2
K_PRECISION = {"split_f16": 2 * 0.922, "split_bf16": 2 * 1.099, "fp32_mfma": 2 * 1.334}
K_FOLD = 2 * 2.567
BUDGET = 2e-4

DEV = "cuda:0"


def _nan_fill(t):
    t.view(torch.int32).fill_(0x7fc00000)


class Stage:
    """one allocation sized for the largest point count, re-carved per case; real parameters and their packed image"""

    def __init__(self, hiplib):
        from dynhor_amd import _lib
        self.L, self._lib = hiplib, _lib
        sdf, col, var = randomized_models(seed=23, device=DEV, jitter=0.05)
        self.flat = flat_from_oracle(sdf, var, col)
        self.packed = torch.empty(hiplib.dh_packed_floats(), device=DEV)
        _lib.check(hiplib.dh_pack_weights(_lib.ptr(self.flat), _lib.ptr(self.packed), _lib.stream()))
        self.big = torch.empty(U.Layout(64 * NT_MAX).total_floats, device=DEV)
        self.grad = torch.empty_like(self.flat)
        self.var = U.variance_offset()

    def carve(self, nt):
        lay = U.Layout(64 * nt)
        assert lay.total_floats == self._lib.workspace_floats(64 * nt)[2]
        return lay, self.big[:lay.total_floats]

    def run(self, arith, lay, ws, what):
        """steps 3..5 of the module docstring; `ws` holds the case's operands, partials and scale words"""
        _lib = self._lib
        _nan_fill(ws[lay.tred: lay.gesave])                         # tred, the DW_G split blocks, the reduced block
        _nan_fill(self.grad)
        before = ws[:lay.tred].clone(), ws[lay.gesave:].clone()
        npts = 64 * lay.ntiles
        _lib.check(self.L.dh_weight_grads_gemm_ex(arith, npts, _lib.ptr(ws), _lib.stream()))
        _lib.check(self.L.dh_weight_grads_fold(_lib.ptr(self.packed), _lib.ptr(self.flat), npts, _lib.ptr(ws), _lib.ptr(self.grad),
                                               _lib.stream()))
        torch.cuda.synchronize()
        # (d) writes stay in their regions
        for name, a, b in (("absmax..tpart", ws[:lay.tred], before[0]), ("gesave", ws[lay.gesave:], before[1])):
            same = a.view(torch.int32) == b.view(torch.int32)
            if not bool(same.all()):
                first = int((~same).nonzero()[0]) + (0 if name != "gesave" else lay.gesave)
                region = [n for n in lay.off if lay.off[n] <= first < lay.off[n] + lay.size[n]]
                raise AssertionError(f"{what}: the stage wrote outside slabs / tred: {int((~same).sum())} words changed, first at float "
                                     f"offset {first} (region {region})")

    def job_matrix(self, lay, ws, job):
        return U.slab_to_matrix(lay.red_job(ws, job), U.DW_NBS[job])

    def tred(self, lay, ws):
        return ws[lay.tred: lay.tred + lay.size["tred"]].view(U.DW_NS, U.N_TILE_PART, 256)


@pytest.fixture(scope="module")
def stage(hiplib):
    return Stage(hiplib)


# ---------------------------------------------------------------- integer operands, written once for NT_MAX tiles
class IntPool:
    def __init__(self):
        g = torch.Generator(device=DEV).manual_seed(1234)
        ri = lambda n: torch.randint(-8, 9, (n,), generator=g, device=DEV).float()
        self.native = {}                                             # (region, layer) -> [NT_MAX * floats per tile], native layout
        for name in INT_REGIONS:
            layers, per = U.REGION_SHAPE[name]
            for l in range(layers):
                self.native[(name, l)] = ri(NT_MAX * per)
        self.tpart = ri(NT_MAX * U.N_TILE_PART * 256)
        self.gesave = ri(NT_MAX * U.TM * 40)
        # int64 reference: per-tile products (fp64 holds them exactly), summed over the first nt tiles by a running sum
        self.cum = []
        for J in U.JOBS:
            P = None
            for a, b in J["pairs"]:
                A = U.native_to_rows(self.native[a]).view(NT_MAX, 64, 256).double()
                B = (U.native_to_rows(self.native[b]) if U.region_width(b[0]) == 256 else U.aux_native_to_rows(self.native[b]))
                B = B.view(NT_MAX, 64, -1).double()
                p = torch.bmm(A.transpose(1, 2), B)
                P = p if P is None else P + p
            self.cum.append(P.round().to(torch.int64).cumsum(0))
        tp = self.tpart.view(NT_MAX, U.N_TILE_PART, 256).to(torch.int64)
        self.tcum = torch.cat([torch.zeros_like(tp[:1]), tp.cumsum(0)])      # [NT_MAX + 1, 20, 256]: sum over tiles < t

    def job_ref(self, job, nt):
        return self.cum[job][nt - 1]

    def tsum_ref(self, nt):
        return self.tcum[nt]

    def write(self, lay, ws, f16_words, tag=True):
        nt = lay.ntiles
        for (name, l), t in self.native.items():
            per = U.REGION_SHAPE[name][1]
            lay.tiles(ws, name, l).copy_(t[:nt * per])
        ws[lay.tpart: lay.tpart + lay.size["tpart"]] = self.tpart[:lay.size["tpart"]]
        ws[lay.gesave: lay.gesave + lay.size["gesave"]] = self.gesave[:lay.size["gesave"]]
        if f16_words:
            U.write_scale_words(lay, ws, tag=tag)
        else:                                                         # the other two forms must not depend on these words
            _nan_fill(ws[lay.absmax: lay.act])


@pytest.fixture(scope="module")
def ints(stage):
    return IntPool()


def _first_bad(bad):
    o, i = (int(v) for v in bad.nonzero()[0])
    return o, i


@pytest.mark.parametrize("nt", NT_SWEEP)
@pytest.mark.parametrize("arith", list(ARITHS))
def test_every_job_equals_the_integer_product(stage, ints, arith, nt):
    lay, ws = stage.carve(nt)
    ints.write(lay, ws, f16_words=arith == "split_f16")
    what = f"arithmetic {arith}, ntiles {nt}"
    stage.run(ARITHS[arith], lay, ws, what)
    for job in range(15):
        got = stage.job_matrix(lay, ws, job).double()
        want = ints.job_ref(job, nt).double()
        bad = ~(got == want)                                          # NaN (an unwritten slab) counts as wrong
        if bool(bad.any()):
            o, i = _first_bad(bad)
            raise AssertionError(f"job {job}, {what}: {int(bad.sum())} of {bad.numel()} elements differ from the int64 product; "
                                 f"first at row {o} col {i}: got {got[o, i].item()} want {want[o, i].item()}")
    # the tile-partial reduction: split s sums tiles [nt s / 64, nt (s + 1) / 64)
    s = torch.arange(U.DW_NS + 1, device=DEV)
    edges = nt * s // U.DW_NS
    want = (ints.tcum[edges[1:]] - ints.tcum[edges[:-1]]).double()
    got = stage.tred(lay, ws).double()
    bad = ~(got == want)
    assert not bool(bad.any()), f"tpart_reduce, {what}: {int(bad.sum())} words differ, first (split, slot, col) {tuple(int(v) for v in bad.nonzero()[0])}"


# ---------------------------------------------------------------- (b) heavy-tailed floats
class FloatCase:
    """row-form operands for `nt` tiles, the fp64 products and the fp32 yardstick, computed once and shared by the arithmetics"""

    def __init__(self, nt):
        g = torch.Generator(device=DEV).manual_seed(500 + nt)
        P = 64 * nt
        self.nt, self.rows, self.zero_tile = nt, {}, {}
        k = 0
        for name in U.OPERAND_REGIONS:
            layers, _ = U.REGION_SHAPE[name]
            for l in range(layers):
                x = torch.randn(P, U.region_width(name), generator=g, device=DEV)
                if name in U.HEAVY:
                    f = torch.exp2(-20.0 * torch.rand(nt, generator=g, device=DEV))
                    z = k % nt                                        # one tile of every heavy class is entirely zero
                    f[z] = 0.0
                    self.zero_tile[(name, l)] = z
                    k += 1
                    x = (x.view(nt, 64, -1) * f[:, None, None]).reshape(P, -1)
                self.rows[(name, l)] = x.contiguous()
        self.tpart = torch.randn(nt * U.N_TILE_PART * 256, generator=g, device=DEV)
        old = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        try:
            self.ref = [U.job_product(j, self.rows, torch.float64) for j in range(15)]
            self.yard = []
            for j in range(15):
                e = (U.job_product(j, self.rows, torch.float32).double() - self.ref[j]).norm() / self.ref[j].norm()
                self.yard.append(float(e))
        finally:
            torch.backends.cuda.matmul.allow_tf32 = old

    def write(self, lay, ws):
        _nan_fill(ws[:lay.tred])                                      # rsave and whatever no case writes: NaN
        for (name, l), x in self.rows.items():
            lay.tiles(ws, name, l).copy_(U.region_to_native(name, x))
        ws[lay.tpart: lay.tpart + lay.size["tpart"]] = self.tpart
        _nan_fill(ws[lay.gesave:])


@pytest.fixture(scope="module")
def float_cases():
    return {}


@pytest.mark.parametrize("nt", [3, 65])
@pytest.mark.parametrize("arith", list(ARITHS))
def test_precision_on_heavy_tailed_operands(stage, float_cases, arith, nt):
    if nt not in float_cases:
        float_cases[nt] = FloatCase(nt)
    case = float_cases[nt]
    lay, ws = stage.carve(nt)
    case.write(lay, ws)
    if arith == "split_f16":
        U.write_scale_words(lay, ws)
    what = f"arithmetic {arith}, ntiles {nt}"
    stage.run(ARITHS[arith], lay, ws, what)
    K = K_PRECISION[arith]
    worst, fails = 0.0, []
    for job in range(15):
        got = stage.job_matrix(lay, ws, job).double()
        assert bool(torch.isfinite(got).all()), f"job {job}, {what}: non-finite slab (zero tiles must contribute nothing, finitely)"
        err = float((got - case.ref[job]).norm() / case.ref[job].norm())
        ratio = err / case.yard[job]
        worst = max(worst, ratio)
        print(f"job {job:2d} {what}: rel Frobenius error {err:.3e}, torch fp32 {case.yard[job]:.3e}, ratio {ratio:.3f}")
        if not (err <= K * case.yard[job] and err <= BUDGET):
            fails.append(f"job {job}, {what}: error {err:.3e} against {K} x {case.yard[job]:.3e} (torch fp32) and the budget {BUDGET}")
    print(f"worst ratio, {what}: {worst:.3f}")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- (c) fold
_fold_refs = {}                                                       # (CPU tensors)


def _fold_ref(ints, stage, nt):
    if nt not in _fold_refs:
        jobs = [ints.job_ref(j, nt).double().cpu() for j in range(15)]
        tsum = ints.tsum_ref(nt).double().cpu()
        flat = stage.flat.cpu()
        _fold_refs[nt] = (U.fold_reference(jobs, tsum, flat), U.fold_reference(jobs, tsum, flat, dtype=torch.float32).double())
    return _fold_refs[nt]


@pytest.mark.parametrize("nt", [1, 33])
@pytest.mark.parametrize("arith", list(ARITHS))
def test_fold_matches_the_fp64_autograd_reference(stage, ints, arith, nt):
    lay, ws = stage.carve(nt)
    ints.write(lay, ws, f16_words=arith == "split_f16")
    what = f"arithmetic {arith}, ntiles {nt}"
    stage.run(ARITHS[arith], lay, ws, what)
    ref64, ref32 = _fold_ref(ints, stage, nt)
    got = stage.grad.double().cpu()
    nan = torch.isnan(got)
    assert bool(nan[stage.var]), f"{what}: the fold wrote the variance slot"
    nan[stage.var] = False
    assert not bool(nan.any()), f"{what}: {int(nan.sum())} parameter slots were not written, first at {int(nan.nonzero()[0])}"
    tensors = U.param_tensors()
    assert dict((n, s) for n, _, s in tensors)["sdf.lin3.weight_v"] == (217, 256)
    assert sum(int(torch.tensor(s).prod()) for _, _, s in tensors) + 1 == got.numel()
    worst, fails = 0.0, []
    for name, off, shape in tensors:
        n = int(torch.tensor(shape).prod())
        r = ref64[off: off + n]
        scale = float(r.abs().max())
        assert scale > 0, name
        err = float((got[off: off + n] - r).abs().max()) / scale
        yard = float((ref32[off: off + n] - r).abs().max()) / scale
        ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"{name:20s} {what}: max error / max {err:.3e}, fp32 reference {yard:.3e}, ratio {ratio:.3f}")
        if not err <= K_FOLD * yard:
            fails.append(f"{name}, {what}: error {err:.3e} against {K_FOLD} x {yard:.3e} (fold_reference in fp32)")
    print(f"worst ratio, {what}: {worst:.3f}")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- (d) on float garbage, (e) the poison contract
@pytest.mark.parametrize("arith", list(ARITHS))
def test_writes_stay_in_their_regions(stage, arith):
    nt = 5
    lay, ws = stage.carve(nt)
    g = torch.Generator(device=DEV).manual_seed(77)
    ws[:lay.tred] = torch.randn(lay.tred, generator=g, device=DEV)
    ws[lay.gesave:] = torch.randn(lay.size["gesave"], generator=g, device=DEV)
    if arith == "split_f16":
        U.write_scale_words(lay, ws)
    stage.run(ARITHS[arith], lay, ws, f"arithmetic {arith}, ntiles {nt}")        # raises when a region changed
    red = ws[lay.red: lay.red + U.GSTRIDE]
    # (a workgroup writes only its own job group's part of its split block, and only that part is read: the rest stays NaN)
    assert bool(torch.isfinite(red).all()) and bool(torch.isfinite(stage.tred(lay, ws)).all())
    assert red.abs().max() > 0


def test_split_f16_without_its_tag_or_with_a_non_finite_class_maximum_writes_nan(stage, ints):
    nt = 3
    lay, ws = stage.carve(nt)
    what = f"arithmetic split_f16, ntiles {nt}"
    ints.write(lay, ws, f16_words=True, tag=False)
    stage.run(ARITHS["split_f16"], lay, ws, what + ", no tag")
    red = ws[lay.red: lay.red + U.GSTRIDE]
    assert bool(torch.isnan(red).all()), f"{what}: {int((~torch.isnan(red)).sum())} slab words look valid without the arithmetic tag"
    assert bool(torch.isnan(stage.grad).any())
    # with the tag, and ABSMAX_ACT = +inf (an activation overflowed the forward chain's constant scale): the jobs that name the
    # class are NaN, the others exact
    ints.write(lay, ws, f16_words=True)
    ws.view(torch.int32)[lay.absmax + U.ABSMAX["act"] * U.ABSMAX_STRIDE] = 0x7f800000
    stage.run(ARITHS["split_f16"], lay, ws, what + ", act maximum +inf")
    for job in range(15):
        got = stage.job_matrix(lay, ws, job)
        names_act = any(U.ABSMAX["act"] in (ca, cb) for ca, _, cb, _ in U.JOB_CLASSES[job])
        if names_act:
            assert bool(torch.isnan(got).all()), f"job {job}, {what}: finite values behind a non-finite activation maximum"
        else:
            assert bool((got.double() == ints.job_ref(job, nt).double()).all()), f"job {job}, {what}: poisoned or wrong without naming the class"
