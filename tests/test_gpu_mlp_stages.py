"""GPU: the four forward MLP stages (SDF no-grad, SDF training forward, input gradient, colour forward) one by one through the stateless
`_ex` entry points, in every arithmetic and chain form, each output and saved tile against the fp64 restatement of THAT stage on THAT
stage's inputs (tests/mlp_stage_util.py; anchored by tests/test_cpu_mlp_stage_ref.py).

Kernels reached (mlp_stage_util.STAGE_KERNELS, printed by the first test): the fp32-MFMA four, the split-bf16 register-resident pair
(chain_t.hip) and its two `_s_` tile chains, the two-piece fp16 register-resident pair (`sdf_*_h_kernel`), its two `_h_` tile chains
and, by DH_CHAIN_FORM_PAIR, the two tile-pair chains.

Sizes: npts in {1, 63, 64, 65, 127, 128, 129, 191, 64 * 7 + 5} -- chain_t.hip works on 128-point workgroup tiles and switches the
second 64-point native tile off when the tile count is odd, the tile forms work on 64-point tiles, the pair forms replay an odd last tile
with its outputs off -- and one looping size per kernel family, where a workgroup takes a second tile (pair) and that pass ends ragged:
32768 + 128 + 5 for the grid-512 tile forms and chain_t's one workgroup per CU, 64 (2 CUs) + 64 * 3 + 5 for the pair forms.

Per case:
 1. VALUES.  Every output and every saved tile (converted to rows; pad rows included, valid columns) under StageLedger's rule:
    max |got - ref64| <= 4 max(e32, ulp) and relative L2 <= 4 max(rel L2 of the fp32 restatement, 2^-24).  Nothing is left out.
 2. PAD ROWS / COLUMNS, CANARY.  The workspace is filled with ray_kernels_util.CANARY_BITS (and stands between two guard pads) before
    every launch.  Afterwards every word of every region the stage owns is written and finite -- the pad rows of a ragged last tile and
    the second 64-point tile of an odd 128-point pair included -- and every other word holds what it held: with save = 0 that is
    everything the stage does not need.  What pads hold, from the code: the SDF forward evaluates pad points at the origin (all pad rows
    of a tile region are bitwise one row); act[3] columns 217..255 hold softplus(0); asave[3]'s hold 0; eaux / caux columns past 39 / 33
    hold 0; caux pad rows are 0; gesave rows are 39 values and one 0, rows past npts are not written.
 3. CLASS WORDS (two-piece fp16, both forms; csrc/workspace.h).  The code's rule, asserted exactly:
      ABSMAX_ASAVE + l = fp32 bits of max |a_l| over the WHOLE tiles of asave[l], pad rows and columns included (lds_handoff's tile
                         maximum, kept as a running maximum per workgroup, one atomicMax each); posted with save != 0 only;
      ABSMAX_CACT + l  = the same over cact[l];   ABSMAX_FEAT = the same over the feature tiles the colour forward READ -- it does
                         NOT take in the extras' maximum (that only joins layer 0's scale);
      ABSMAX_CAUX      = max(1, |p|, |d|, |n|) over the VALID rows: floored at 1 for the sines and cosines, so it is at least the
                         maximum of the written caux region (whose pad rows are 0) but not always in its binade;
      ABSMAX_ACT       = the maximum over the whole act region, posted by the input gradient at every save;
    so each word is at least the maximum of its class's whole written region and (all but CAUX's floor) equal to it: the condition the
    weight-gradient kernel's fp16 split depends on.  Every arithmetic's dh_sdf_forward_ex clears the whole table, which the test filled
    with garbage; only the fp16 arithmetic leaves ABSMAX_TAG_F16.
 4. REPEATABILITY.  A second launch on a fresh canary workspace gives the same bits, outputs and workspace.

Inputs.  SDF forward: points in [-1.2, 1.2]^3 with the origin, points on the box faces and one coordinate exactly 0.0 planted; the
training forward's and the no-grad chain's sdf are judged against one reference.  Input gradient: once on the act tiles the same
arithmetic's forward saved (read back, the reference is fed the same bits), once on planted tiles that span sigma' per layer (+0, 1e-9,
ln 2 / 100, 0.05, 1, 40 -- there sigma' is exactly 1 -- and random values); save in {0, 1, 2}.  Colour forward: planted feature tiles
and normals (norm 0 and norm 50 among them), n_per_ray in {1, 4, 64, 100, 128, npts + 7}, save in {0, 1}; pts, dirs and normals are
allocated at exactly their valid length with a run of NaN behind each.

Measured on MI355X (worst err / bound, worst relative L2 over every size, seed and output; printed by each test):
    SDF forward / no-grad   fp32_mfma 0.424, 1.16e-6   split_bf16 0.395, 9.9e-7    split_f16 0.454, 6.7e-7
    input gradient          fp32_mfma 0.613, 2.07e-6   split_bf16 0.494, 2.03e-6   split_f16 tile and pair 0.443, 2.32e-6
    colour forward          fp32_mfma 0.389, 3.6e-7    split_bf16 0.394, 3.5e-7    split_f16 tile and pair 0.300, 3.0e-7
No output needed a bound other than the rule's.  The file takes about 5 s inside the suite.
"""
import functools
import math
import os
import re

import pytest
import torch

from tests import mlp_stage_util as S
from tests.dw_util import ABSMAX, ABSMAX_FLOATS, ABSMAX_STRIDE, ABSMAX_TAG_F16, TM, Layout
from tests.ray_kernels_util import CANARY_BITS, F32, F64, PAD, Canary
from tests.util import flat_from_oracle, randomized_models

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = (0, 1)
SMALL = (1, 63, 64, 65, 127, 128, 129, 191, 64 * 7 + 5)
LOOP_TILE = 32768 + 128 + 5
ARITHS = (S.FP32, S.BF16, S.F16)


def _loop_size(form):
    if form == S.FORM_PAIR:
        return 64 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 64 * 3 + 5
    return LOOP_TILE


# ------------------------------------------------------------------------------------------------ fixtures of the module
@functools.lru_cache(maxsize=None)
def _net(seed):
    """(flat, packed, fp64 weights, fp32 weights) of one jittered model; packed once"""
    from dynhor_amd import _lib
    sdf, col, var = randomized_models(seed=seed, device=DEV, jitter=0.05)
    flat = flat_from_oracle(sdf, var, col)
    packed = torch.empty(_lib.lib().dh_packed_floats(), device=DEV)
    _lib.check(_lib.lib().dh_pack_weights(_lib.ptr(flat), _lib.ptr(packed), _lib.stream()))
    torch.cuda.synchronize()
    return flat, packed, S.Weights(flat, F64), S.Weights(flat, F32)


def _call(name, *args):
    from dynhor_amd import _lib
    conv = [_lib.ptr(a) if torch.is_tensor(a) else a for a in args]
    _lib.check(getattr(_lib.lib(), name)(*conv, _lib.stream()))
    torch.cuda.synchronize()


def _exact_length(x):
    """x on the device at exactly its length, a run of NaN behind it: a read past the end shows in the outputs"""
    buf = torch.full((x.numel() + 64,), float("nan"), device=DEV)
    buf[: x.numel()] = x.reshape(-1).to(DEV)
    return buf[: x.numel()].view(x.shape)


@functools.lru_cache(maxsize=None)
def _points(npts, seed):
    g = torch.Generator().manual_seed(1000 * seed + npts)
    p = (torch.rand(npts, 3, generator=g) * 2 - 1) * 1.2
    p[0] = 0.0                                                       # the origin
    if npts > 8:
        p[1, 0], p[2, 1], p[3, 2] = 1.2, -1.2, 1.2                   # on the box faces
        p[4, 1] = 0.0                                                # one coordinate exactly 0.0
        p[npts - 1] = torch.tensor([-1.2, 1.2, -1.2])                # a corner, last row of the ragged tile
    return _exact_length(p)


class Work:
    """a canary-filled workspace of fwd_floats (or total_floats) between two guard pads"""

    def __init__(self, npts, total=False):
        self.lay = Layout(npts)
        self.n = self.lay.total_floats if total else self.lay.fwd_floats
        self.raw = torch.full((PAD + self.n + PAD,), CANARY_BITS, dtype=torch.int32, device=DEV)
        self.bits = self.raw[PAD: PAD + self.n]
        self.f = self.bits.view(F32)
        self.before = None

    def zero_table(self):
        """what every training forward does first (launch_sdf_fwd_train): the stages behind it raise the words with atomicMax"""
        self.bits[self.lay.absmax: self.lay.absmax + ABSMAX_FLOATS] = 0

    def snapshot(self):
        self.before = self.raw.clone()

    def region(self, name):
        a, b = S.region_range(self.lay, name)
        return (PAD + a, PAD + b)

    def word(self, cls):
        a = PAD + self.lay.absmax + cls * ABSMAX_STRIDE
        return (a, a + 1)

    def check(self, led, case, owned):
        S.check_canary(led, case, self.raw, self.before, owned)


def _words_by_rule(led, case, w, expect):
    """expect: {class: (region maximum, exact value or None)}"""
    for cls, (mx, exact) in expect.items():
        word = S.absmax_word(w.lay, w.f, cls)
        led.expect(S.class_word_ok(word, mx, exact=mx if exact is None else exact),
                   f"{case}: class word {cls} = {word:#010x}, region maximum {float(mx):.9g} ({S.float_bits(mx):#010x})"
                   + ("" if exact is None else f", rule gives {float(exact):.9g}"))


def _region_max(w, name, layer):
    return w.lay.tiles(w.f, name, layer).abs().max().item()


# ------------------------------------------------------------------------------------------------ the table
def test_the_table_names_a_kernel_for_every_entry_point_arithmetic_and_form():
    src = ""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynhor_amd", "csrc")
    for f in ("kernels_mlp.hip", "kernels_mlp_h.hip", "chain_t.hip", "chain_pair.hip"):
        with open(os.path.join(root, f)) as fh:
            src += fh.read()
    print("entry point, arithmetic / form -> kernel")
    for (entry, arith, form), kernel in S.STAGE_KERNELS.items():
        print(f"  {entry:22s} {S.form_label(arith, form):16s} {kernel}")
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", src), kernel
    assert len(set(S.STAGE_KERNELS.values())) == len(S.STAGE_KERNELS) == 14


# ------------------------------------------------------------------------------------------------ SDF forward / no-grad
@functools.lru_cache(maxsize=None)
def _forward_refs(seed, npts):
    _, _, W64, W32 = _net(seed)
    pad = Layout(npts).ntiles * TM - npts
    pts = _points(npts, seed)
    return S.sdf_forward_ref(W64, pts, pad_rows=pad), S.sdf_forward_ref(W32, pts, pad_rows=pad)


def _run_forward(arith, seed, npts, garbage=True):
    _, packed, _, _ = _net(seed)
    pts = _points(npts, seed)
    w = Work(npts)
    if garbage:
        w.bits[w.lay.absmax: w.lay.absmax + ABSMAX_FLOATS] = torch.randint(-2 ** 31, 2 ** 31 - 1, (ABSMAX_FLOATS,), dtype=torch.int64,
                                                                         generator=torch.Generator().manual_seed(npts)).to(torch.int32).to(DEV)
    w.snapshot()
    c = Canary(DEV)
    sdf = c.out("sdf", npts)
    _call("dh_sdf_forward_ex", arith, packed, pts, npts, w.f, sdf)
    c.check()
    return w, sdf


def _check_forward(led, arith, seed, npts):
    case = f"{S.ARITH_LABEL[arith]} seed {seed} npts {npts}"
    _, packed, _, _ = _net(seed)
    pts = _points(npts, seed)
    w, sdf = _run_forward(arith, seed, npts)
    lay = w.lay
    table = (PAD + lay.absmax, PAD + lay.absmax + ABSMAX_FLOATS)
    w.check(led, case, [table, w.region("act"), w.region("eaux"), w.region("feat")])
    tab = w.bits[lay.absmax: lay.absmax + ABSMAX_FLOATS].clone()
    tag = int(tab[ABSMAX["tag"] * ABSMAX_STRIDE].item())
    led.expect(tag == (ABSMAX_TAG_F16 if arith == S.F16 else 0), f"{case}: arithmetic tag {tag:#x}")
    tab[ABSMAX["tag"] * ABSMAX_STRIDE] = 0
    led.expect(not bool(tab.any()), f"{case}: {int((tab != 0).sum())} words of the class table were not cleared")
    r64, r32 = _forward_refs(seed, npts)
    led.add("sdf", sdf, r64["sdf"][:npts], r32["sdf"][:npts], case)
    c = Canary(DEV)
    sdf_ng = c.out("sdf_nograd", npts)
    _call("dh_sdf_nograd_ex", arith, packed, pts, npts, sdf_ng)
    c.check()
    led.add("sdf_nograd", sdf_ng, r64["sdf"][:npts], r32["sdf"][:npts], case)
    for name, layers in (("act", 8), ("feat", 1), ("eaux", 1)):
        for l in range(layers):
            rows = S.region_rows(lay, w.f, name, l)
            pick = lambda r: r[name][l] if name == "act" else r[name]
            S.judge_tile_rows(led, name, l, case, rows, pick(r64), pick(r32))
            if rows.shape[0] - npts >= 2:                            # every pad row is the origin's row, bit for bit
                padr = rows[npts:].view(torch.int32)
                led.expect(bool((padr == padr[:1]).all()), f"{case}: pad rows of {name}[{l}] differ from one another")
    # 4. the same bits again
    w2, sdf2 = _run_forward(arith, seed, npts)
    led.expect(torch.equal(w2.bits, w.bits) and torch.equal(sdf2.view(torch.int32), sdf.view(torch.int32)), f"{case}: forward not repeatable")
    c = Canary(DEV)
    ng2 = c.out("sdf_nograd", npts)
    _call("dh_sdf_nograd_ex", arith, packed, pts, npts, ng2)
    led.expect(torch.equal(ng2.view(torch.int32), sdf_ng.view(torch.int32)), f"{case}: no-grad chain not repeatable")


@pytest.mark.parametrize("arith", ARITHS, ids=[S.ARITH_LABEL[a] for a in ARITHS])
def test_sdf_forward_and_nograd(hiplib, arith):
    led = S.StageLedger()
    for seed in SEEDS:
        for npts in SMALL:
            _check_forward(led, arith, seed, npts)
    _check_forward(led, arith, SEEDS[0], LOOP_TILE)
    led.report(f"SDF forward / no-grad, {S.ARITH_LABEL[arith]}")
    led.check()


# ------------------------------------------------------------------------------------------------ input gradient
def _planted_act(seed, npts):
    """whole tiles of act[0..7] that span sigma' = 1 - exp(-100 h) per layer; act[3]'s pad columns as the forward leaves them"""
    g = torch.Generator().manual_seed(77 * seed + npts)
    R = Layout(npts).ntiles * TM
    special = torch.tensor([0.0, 1e-9, math.log(2.0) / 100.0, 0.05, 1.0, 40.0])
    out = []
    for l in range(8):
        h = torch.rand(R, 256, generator=g) ** 3 * 0.3                         # most mass where sigma' bends
        idx = torch.randint(0, 6, (R, 256), generator=g)
        h = torch.where(torch.rand(R, 256, generator=g) < 0.25, special[idx], h)
        h[:, l] = special[(torch.arange(R) + l) % 6]                           # every special value in every layer at every size
        if l == 3:
            h[:, 217:] = S.SOFTPLUS0
        out.append(h.to(DEV))
    return out


def _check_gradient(led, arith, form, seed, npts, sources=("saved", "planted"), saves=(1, 0, 2)):
    from dynhor_amd import _lib
    _, packed, W64, W32 = _net(seed)
    pts = _points(npts, seed)
    limit = _lib.range_words()[2]
    for source in sources:
        if source == "saved":
            wf, _ = _run_forward(arith, seed, npts, garbage=False)
            act = [S.region_rows(wf.lay, wf.f, "act", l).clone() for l in range(8)]
            del wf
        else:
            act = _planted_act(seed, npts)
            assert max(h.max().item() for h in act) < limit
        g64, g32 = S.sdf_gradient_ref(W64, pts, act), S.sdf_gradient_ref(W32, pts, act)
        act_max = max(h.max().item() for h in act)
        for save in saves:
            case = f"{S.form_label(arith, form)} seed {seed} npts {npts} {source} act save {save}"

            def launch():
                w = Work(npts, total=(save == 2))
                w.zero_table()
                for l in range(8):
                    S.write_region_rows(w.lay, w.f, "act", l, act[l])
                w.snapshot()
                c = Canary(DEV)
                n = c.out("normals", npts, 3)
                _call("dh_sdf_gradient_ex", arith | form, packed, pts, npts, w.f, n, save)
                c.check()
                return w, n
            w, normals = launch()
            lay = w.lay
            owned = [w.region("asave")] if save else []
            if save == 2:
                owned.append((PAD + lay.gesave, PAD + lay.gesave + npts * 40))
            if arith == S.F16:
                owned += [w.word(ABSMAX["act"])] + ([w.word(ABSMAX["asave"] + l) for l in range(8)] if save else [])
            w.check(led, case, owned)
            led.add("normals", normals, g64["normals"], g32["normals"], case)
            if save:
                for l in range(8):
                    S.judge_tile_rows(led, "asave", l, case, S.region_rows(lay, w.f, "asave", l), g64["a"][l], g32["a"][l])
            if save == 2:
                ge = w.f[lay.gesave: lay.gesave + npts * 40].view(npts, 40)
                led.add("gesave", ge[:, :39], g64["ge"], g32["ge"], case)
                led.expect(bool((ge[:, 39] == 0).all()), f"{case}: gesave column 39 is not zero")
            if arith == S.F16:
                expect = {ABSMAX["act"]: (act_max, None)}
                if save:
                    expect.update({ABSMAX["asave"] + l: (_region_max(w, "asave", l), None) for l in range(8)})
                _words_by_rule(led, case, w, expect)
            w2, n2 = launch()
            led.expect(torch.equal(w2.bits, w.bits) and torch.equal(n2.view(torch.int32), normals.view(torch.int32)), f"{case}: not repeatable")


@pytest.mark.parametrize("arith,form", S.CHAIN_FORMS, ids=[S.form_label(a, f) for a, f in S.CHAIN_FORMS])
def test_input_gradient(hiplib, arith, form):
    led = S.StageLedger()
    for seed in SEEDS:
        for npts in SMALL:
            _check_gradient(led, arith, form, seed, npts)
    _check_gradient(led, arith, form, SEEDS[0], _loop_size(form), sources=("saved",), saves=(1,))
    led.report(f"input gradient, {S.form_label(arith, form)}")
    led.check()


# ------------------------------------------------------------------------------------------------ colour forward
def _colour_inputs(seed, npts, n_per_ray):
    g = torch.Generator().manual_seed(13 * seed + 1000 * n_per_ray + npts)
    R = Layout(npts).ntiles * TM
    nrays = (npts + n_per_ray - 1) // n_per_ray
    dirs = torch.nn.functional.normalize(torch.randn(nrays, 3, generator=g), dim=-1)
    normals = torch.nn.functional.normalize(torch.randn(npts, 3, generator=g), dim=-1) * (0.6 + 0.8 * torch.rand(npts, 1, generator=g))
    normals[torch.arange(npts) % 13 == 5] = 0.0                                 # norm 0
    big = torch.arange(npts) % 67 == 11                                          # norm 50: the extras' class maximum follows it
    normals[big] = torch.nn.functional.normalize(normals[big] + 1e-3, dim=-1) * 50.0
    feat = torch.randn(R, 256, generator=g) * 0.5                                # whole tiles, pad rows included
    return _exact_length(dirs), _exact_length(normals), feat.to(DEV)


def _check_colour(led, arith, form, seed, npts, n_per_ray, saves=(1, 0)):
    _, packed, W64, W32 = _net(seed)
    pts = _points(npts, seed)
    dirs, normals, feat = _colour_inputs(seed, npts, n_per_ray)
    pad = feat.shape[0] - npts
    c64 = S.color_forward_ref(W64, pts, dirs, n_per_ray, normals, feat, pad_rows=pad)
    c32 = S.color_forward_ref(W32, pts, dirs, n_per_ray, normals, feat, pad_rows=pad)
    extras_max = max(1.0, pts.abs().max().item(), dirs.abs().max().item(), normals.abs().max().item())
    for save in saves:
        case = f"{S.form_label(arith, form)} seed {seed} npts {npts} n_per_ray {n_per_ray} save {save}"

        def launch():
            w = Work(npts)
            w.zero_table()
            S.write_region_rows(w.lay, w.f, "feat", 0, feat)
            w.snapshot()
            c = Canary(DEV)
            col = c.out("colour", npts, 3)
            _call("dh_color_forward_ex", arith | form, packed, pts, dirs, n_per_ray, normals, npts, w.f, col, save)
            c.check()
            return w, col
        w, colour = launch()
        lay = w.lay
        owned = [w.region("cact"), w.region("caux")] if save else []
        if arith == S.F16 and save:
            owned += [w.word(ABSMAX["cact"] + l) for l in range(4)] + [w.word(ABSMAX["feat"]), w.word(ABSMAX["caux"])]
        w.check(led, case, owned)
        led.add("colour", colour, c64["color"], c32["color"], case)
        if save:
            for l in range(4):
                S.judge_tile_rows(led, "cact", l, case, S.region_rows(lay, w.f, "cact", l), c64["cact"][l], c32["cact"][l])
            S.judge_tile_rows(led, "caux", 0, case, S.region_rows(lay, w.f, "caux", 0), c64["caux"], c32["caux"], npts=npts)
            if arith == S.F16:
                expect = {ABSMAX["cact"] + l: (_region_max(w, "cact", l), None) for l in range(4)}
                expect[ABSMAX["feat"]] = (feat.abs().max().item(), None)
                expect[ABSMAX["caux"]] = (_region_max(w, "caux", 0), extras_max)
                _words_by_rule(led, case, w, expect)
        w2, col2 = launch()
        led.expect(torch.equal(w2.bits, w.bits) and torch.equal(col2.view(torch.int32), colour.view(torch.int32)), f"{case}: not repeatable")


@pytest.mark.parametrize("arith,form", S.CHAIN_FORMS, ids=[S.form_label(a, f) for a, f in S.CHAIN_FORMS])
def test_colour_forward(hiplib, arith, form):
    led = S.StageLedger()
    for i, npts in enumerate(SMALL):
        for j, n_per_ray in enumerate((1, 4, 64, 100, 128, npts + 7)):
            _check_colour(led, arith, form, SEEDS[(i + j) % 2], npts, n_per_ray)
    _check_colour(led, arith, form, SEEDS[0], _loop_size(form), 128, saves=(1,))
    led.report(f"colour forward, {S.form_label(arith, form)}")
    led.check()


# ------------------------------------------------------------------------------------------------ the class words of a whole forward
@pytest.mark.parametrize("form", [S.FORM_TILE, S.FORM_PAIR], ids=["tile", "pair"])
def test_class_words_after_forward_gradient_colour(hiplib, form):
    """forward -> input gradient -> colour forward on ONE workspace whose table held garbage: all fourteen words by the rule of the
    module docstring (no stage disturbs another's words), the tag, and nothing else in the table."""
    led = S.StageLedger()
    for seed, npts, n_per_ray in ((0, 65, 4), (1, 64 * 7 + 5, 128), (0, 1, 1), (1, 191, 64)):
        case = f"split_f16{'/tile' if form == S.FORM_TILE else '/pair'} seed {seed} npts {npts}"
        _, packed, _, _ = _net(seed)
        pts = _points(npts, seed)
        dirs, _, _ = _colour_inputs(seed, npts, n_per_ray)
        w, _ = _run_forward(S.F16, seed, npts, garbage=True)
        normals = torch.empty(npts, 3, device=DEV)
        colour = torch.empty(npts, 3, device=DEV)
        _call("dh_sdf_gradient_ex", S.F16 | form, packed, pts, npts, w.f, normals, 1)
        _call("dh_color_forward_ex", S.F16 | form, packed, pts, dirs, n_per_ray, normals, npts, w.f, colour, 1)
        expect = {ABSMAX["asave"] + l: (_region_max(w, "asave", l), None) for l in range(8)}
        expect.update({ABSMAX["cact"] + l: (_region_max(w, "cact", l), None) for l in range(4)})
        expect[ABSMAX["feat"]] = (_region_max(w, "feat", 0), None)
        expect[ABSMAX["act"]] = (max(_region_max(w, "act", l) for l in range(8)), None)
        expect[ABSMAX["caux"]] = (_region_max(w, "caux", 0),
                                  max(1.0, pts.abs().max().item(), dirs.abs().max().item(), normals.abs().max().item()))
        _words_by_rule(led, case, w, expect)
        tab = w.bits[w.lay.absmax: w.lay.absmax + ABSMAX_FLOATS].clone()
        led.expect(int(tab[ABSMAX["tag"] * ABSMAX_STRIDE].item()) == ABSMAX_TAG_F16, f"{case}: no arithmetic tag")
        for cls in list(expect) + [ABSMAX["tag"]]:
            tab[cls * ABSMAX_STRIDE] = 0
        led.expect(not bool(tab.any()), f"{case}: {int((tab != 0).sum())} other words of the table are set")
    led.check()
