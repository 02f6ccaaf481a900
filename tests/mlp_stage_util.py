"""Plain restatements of the four forward MLP stages (SDF no-grad / training forward, input gradient, colour forward: csrc/kernels_mlp.hip,
kernels_mlp_h.hip, chain_t.hip, chain_pair.hip) for the tests that drive each stage alone (tests/test_gpu_mlp_stages.py; anchored on
the CPU by tests/test_cpu_mlp_stage_ref.py).

Nothing here launches a kernel; every function works on CPU or GPU tensors in the dtype it is asked for (fp64: the reference; fp32: the
yardstick of the acceptance criterion).  The effective weights come from the flat parameter vector, W = g v / |v| formed in that dtype,
never from the packed image the kernels read.  Every restatement takes the STAGE's own inputs and returns every output in row form
([points, features]); the tile <-> row conversions, the workspace carving and the class-word numbering are tests/dw_util.py's.

  sdf_forward_ref   pts                                   -> sdf, feat (lin8 rows 1..256), act[0..7] (softplus beta = 100), eaux [P, 39]
  sdf_gradient_ref  pts, act[0..7] AS GIVEN               -> normals, a_0..a_7, ge
  color_forward_ref pts, dirs, n_per_ray, normals, feat   -> caux [P, 33], cact[0..3] (ReLU), colour = sigmoid(lin4)

pad_rows: the kernels work on whole 64-point tiles.  The SDF forward evaluates the pad points of a ragged last tile at the origin
(mlp_common.h embed_tile, chain_t.hip: x = 0 where the point index is past the end); the colour forward gives them zero extras (all 33
columns: not the extras of a point at the origin, whose cosines would be 1) and whatever the feature tile holds in those rows.  The
restatements append exactly these rows, so that a pad row is judged like any other.

The acceptance criterion (StageLedger, judge): tests/ray_kernels_util.py ErrorLedger's element rule
    max |got - ref64| <= 4 max(e32, ulp)       e32 = max |ref32 - ref64| on the same inputs, ulp = one fp32 ulp of the largest element
and a relative L2 bounded by 4 x max(the fp32 restatement's relative L2, U32) instead of the ledger's fixed 1e-4.
"""
import math

import torch

from tests.dw_util import (ABSMAX_STRIDE, CAUX, EMB, N_COL, N_SDF, SKIP_OUT, aux_native_to_rows, aux_rows_to_native, native_to_rows,
                           param_tensors, region_width, rows_to_native)
from tests.ray_kernels_util import CANARY_BITS, F32, F64, U32, ErrorLedger, measure

BETA = 100.0
SOFTPLUS0 = math.log(2.0) / BETA          # softplus(0): what act[3]'s columns 217..255 hold (zero weight rows, zero bias)
RSQRT2 = 1.0 / math.sqrt(2.0)
MARGIN = 4.0                              # the project's margin (ErrorLedger); also tile16h.h's 2^-22 |X| over fp32's 2^-24

BF16, FP32, F16 = 0, 1, 2                 # include/dynhor_hip.h dh_arithmetic
FORM_TILE, FORM_PAIR = 0x100, 0x200       # DH_CHAIN_FORM_*

# (entry point, arithmetic, form) -> the kernel that runs it (csrc/kernels_mlp.hip launch_*, chain_t.hip, kernels_mlp_h.hip, chain_pair.hip)
STAGE_KERNELS = {
    ("dh_sdf_nograd_ex", FP32, 0): "sdf_nograd_kernel", ("dh_sdf_forward_ex", FP32, 0): "sdf_fwd_train_kernel",
    ("dh_sdf_gradient_ex", FP32, 0): "sdf_grad_kernel", ("dh_color_forward_ex", FP32, 0): "color_fwd_kernel",
    ("dh_sdf_nograd_ex", BF16, 0): "sdf_nograd_t_kernel", ("dh_sdf_forward_ex", BF16, 0): "sdf_fwd_train_t_kernel",
    ("dh_sdf_gradient_ex", BF16, 0): "sdf_grad_s_kernel", ("dh_color_forward_ex", BF16, 0): "color_fwd_s_kernel",
    ("dh_sdf_nograd_ex", F16, 0): "sdf_nograd_h_kernel", ("dh_sdf_forward_ex", F16, 0): "sdf_fwd_train_h_kernel",
    ("dh_sdf_gradient_ex", F16, FORM_TILE): "sdf_grad_h_kernel", ("dh_color_forward_ex", F16, FORM_TILE): "color_fwd_h_kernel",
    ("dh_sdf_gradient_ex", F16, FORM_PAIR): "sdf_grad_p_kernel", ("dh_color_forward_ex", F16, FORM_PAIR): "color_fwd_p_kernel",
}
ARITH_LABEL = {FP32: "fp32_mfma", BF16: "split_bf16", F16: "split_f16"}
# the (arithmetic, form) pairs of the two stages that have a pair form
CHAIN_FORMS = ((FP32, 0), (BF16, 0), (F16, FORM_TILE), (F16, FORM_PAIR))


def form_label(arith, form):
    return ARITH_LABEL[arith] + {0: "", FORM_TILE: "/tile", FORM_PAIR: "/pair"}[form]


# ------------------------------------------------------------------------------------------------ weights
class Weights:
    """.sdf[l] = (W [out, in], b [out]) of SDF lin0..8, .col[l] of colour lin0..4, W = g v / |v| in `dtype` on `device`."""

    def __init__(self, flat, dtype, device=None):
        device = flat.device if device is None else device
        p = flat.detach().to(device=device, dtype=dtype)
        lay = param_tensors()
        lins = []
        for k in range(N_SDF + N_COL):
            (_, boff, (od,)), (_, goff, _), (_, voff, (_, idim)) = lay[3 * k: 3 * k + 3]
            g = p[goff: goff + od].reshape(od, 1)
            v = p[voff: voff + od * idim].reshape(od, idim)
            lins.append((g * v / v.norm(dim=1, keepdim=True), p[boff: boff + od]))
        self.sdf, self.col = lins[:N_SDF], lins[N_SDF:]
        self.dtype, self.device = dtype, device


# ------------------------------------------------------------------------------------------------ the stages
def embed6(x):
    """[x, sin(2^k x), cos(2^k x)]_{k < 6}: 39 wide"""
    out = [x]
    for k in range(6):
        out += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
    return torch.cat(out, -1)


def sdf_forward_ref(W, pts, pad_rows=0):
    """act[3] is returned 217 wide (its valid columns)."""
    x = pts.to(device=W.device, dtype=W.dtype)
    if pad_rows:
        x = torch.cat([x, x.new_zeros(pad_rows, 3)])
    e = embed6(x)
    h, act = e, []
    for l in range(8):
        Wl, bl = W.sdf[l]
        if l == 4:
            h = torch.cat([h, e], 1) * RSQRT2
        h = torch.nn.functional.softplus(h @ Wl.t() + bl, beta=BETA)
        act.append(h)
    y = h @ W.sdf[8][0].t() + W.sdf[8][1]
    return {"sdf": y[:, 0], "feat": y[:, 1:], "act": act, "eaux": e}


def softplus_deriv_from_h(h):
    """sigma'(z) from h = softplus(z): 1 - exp(-beta h)   (csrc/tile.h softplus_deriv_from_h, DESIGN.md "Backward math")"""
    return 1.0 - torch.exp(-BETA * h)


def sdf_gradient_ref(W, pts, act):
    """pts [P, 3]; act[l] [R, >= width of layer l] with R >= P (whole tiles: the rows past P are the pad rows of the a_l tiles).
    Returns normals [P, 3], ge [P, 39], a[0..7] ([R, 256]; a[3] is [R, 217])."""
    x = pts.to(device=W.device, dtype=W.dtype)
    P = x.shape[0]
    act = [h.to(device=W.device, dtype=W.dtype) for h in act]
    a = [None] * 8
    a[7] = W.sdf[8][0][0][None, :] * softplus_deriv_from_h(act[7])
    ge = None
    for l in range(7, 0, -1):
        u = a[l] @ W.sdf[l][0]
        if l == 4:
            ge = u[:, SKIP_OUT:] * RSQRT2
            u = u[:, :SKIP_OUT] * RSQRT2
        a[l - 1] = u * softplus_deriv_from_h(act[l - 1][:, : u.shape[1]])
    ge = (ge + a[0] @ W.sdf[0][0])[:P]
    n = ge[:, 0:3].clone()
    for k in range(6):
        f = float(2 ** k)
        n = n + f * (torch.cos(x * f) * ge[:, 3 + 6 * k: 6 + 6 * k] - torch.sin(x * f) * ge[:, 6 + 6 * k: 9 + 6 * k])
    return {"normals": n, "ge": ge, "a": a}


def color_extras(pts, dirs, n_per_ray, normals):
    """caux = [p, d, sin / cos (2^k d) for k < 4, n]: 33 wide; point i belongs to ray i // n_per_ray"""
    P = pts.shape[0]
    d = dirs[torch.arange(P, device=pts.device) // n_per_ray]
    out = [pts, d]
    for k in range(4):
        out += [torch.sin(d * float(2 ** k)), torch.cos(d * float(2 ** k))]
    return torch.cat(out + [normals], -1)


def color_forward_ref(W, pts, dirs, n_per_ray, normals, feat, pad_rows=0):
    """feat [P + pad_rows, 256]; the pad rows get zero extras."""
    c = lambda t: t.to(device=W.device, dtype=W.dtype)
    caux = color_extras(c(pts), c(dirs), n_per_ray, c(normals))
    if pad_rows:
        caux = torch.cat([caux, caux.new_zeros(pad_rows, CAUX)])
    h = torch.cat([caux, c(feat)], 1)
    cact = []
    for l in range(4):
        h = torch.relu(h @ W.col[l][0].t() + W.col[l][1])
        cact.append(h)
    colour = torch.sigmoid(h @ W.col[4][0].t() + W.col[4][1])
    return {"caux": caux, "cact": cact, "color": colour[: pts.shape[0]]}


# ------------------------------------------------------------------------------------------------ the criterion
def rel_l2(x, ref64):
    ref64 = ref64.to(F64)
    nrm = ref64.norm().item()
    d = (x.to(F64) - ref64).norm().item()
    return d / nrm if nrm > 0 else (0.0 if d == 0 else float("inf"))


def judge(got, ref64, ref32):
    """(ok, err / bound, relative L2 / its bound, text).  Nothing is left out: every element of `got`, which must be finite."""
    if got.shape != ref64.shape:
        return False, float("inf"), float("inf"), f"shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    if not bool(torch.isfinite(got).all()):
        return False, float("inf"), float("inf"), f"{int((~torch.isfinite(got)).sum())} non-finite elements"
    err, e32, ulp, rel = measure(got, ref64, ref32)
    bound = MARGIN * max(e32, ulp)
    rbound = MARGIN * max(rel_l2(ref32, ref64), U32)
    r1 = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    r2 = rel / rbound
    text = (f"max err {err:.3e} vs {MARGIN:g} x max(fp32 {e32:.3e}, ulp {ulp:.3e}) = {bound:.3e}; "
            f"rel L2 {rel:.3e} vs bound {rbound:.3e}")
    return (err <= bound and rel <= rbound), r1, r2, text


class StageLedger(ErrorLedger):
    """ErrorLedger's element rule with the relative-L2 bound taken from the fp32 restatement (judge).  A miss is recorded, not raised,
    so that one run reports every output of every case; check() asserts that nothing was recorded."""

    def __init__(self):
        super().__init__(rel_tol=None)
        self.failures = []

    def add(self, name, got, ref64, ref32, case="", pool=False):
        assert not pool
        ok, r1, r2, text = judge(got, ref64, ref32)
        w = self.worst.get(name)
        if w is None or r1 > w[0]:
            self.worst[name] = (r1, text, case)
        rel = rel_l2(got, ref64) if got.shape == ref64.shape else float("inf")
        w = self.worst.get(name + "/rel")
        self.worst[name + "/rel"] = (max(r2, w[0]), max(rel, w[1])) if w else (r2, rel)
        if not ok:
            self.failures.append(f"{name} [{case}]: {text}")

    def fail(self, text):
        self.failures.append(text)

    def expect(self, cond, text):
        if not bool(cond):
            self.failures.append(text)

    def report(self, title):
        rows = [(k, w, self.worst[k + "/rel"]) for k, w in self.worst.items() if not k.endswith("/rel")]
        print(f"\n{title}: worst err/bound {max(w[0] for _, w, _ in rows):.3f}, worst relative L2 {max(r[1] for _, _, r in rows):.2e} "
              f"(at most {max(r[0] for _, _, r in rows):.3f} of its bound)")
        for k, w, r in rows:
            print(f"  {k:10s} worst err/bound {w[0]:.3f} [{w[2]}]  ({w[1]});  worst rel L2 {r[1]:.2e}, of its bound {r[0]:.3f}")

    def check(self):
        assert not self.failures, f"{len(self.failures)} misses:\n" + "\n".join(self.failures[:40])


def float_bits(x):
    """fp32 bit pattern of a python float / 0-dim tensor as an int"""
    return int(torch.as_tensor(float(x), dtype=F32).reshape(1).view(torch.int32).item()) & 0xFFFFFFFF


def class_word_ok(word, region_max, exact=None):
    """The condition the weight-gradient kernel's fp16 split depends on: the word (fp32 bits) is at least the fp32 bits of max |x| over
    the whole written region of its class and lies in the same binade; `exact`: the value the code's rule makes the word equal to
    (then equality is asked and the binade condition applies to that value: ABSMAX_CAUX is floored at 1)."""
    word = int(word) & 0xFFFFFFFF
    m = float_bits(region_max)
    if exact is not None:
        return word == float_bits(exact) and word >= m
    return word >= m and (word >> 23) == (m >> 23)


# valid columns of a saved region's rows (the others are pad columns with a value the code fixes)
def valid_width(name, layer):
    if name in ("act", "asave") and layer == 3:
        return SKIP_OUT
    return {"eaux": EMB, "caux": CAUX}.get(name, 256)


def judge_tile_rows(led, name, layer, case, got, ref64, ref32, npts=None):
    """One layer of a saved region in row form, whole tiles ([ntiles * 64, 256 or 64]) against the restatements' rows (same row count,
    valid columns only).  Valid columns by the ledger's rule, pad rows included; pad columns exactly as the code leaves them:
      act[3] 217..255   softplus(0) = ln 2 / 100: zero weight rows and zero bias.  The tile chains store fp32(softplus100(0)), chain_t
                        stores the constant fp32(ln 2 / 100) in columns 224..255 and (hi + lo) / 16 of its two fp16 pieces below:
                        one fp32 rounding of the constant (U32) and the two-piece representation (2^-22 = 4 U32) -> 5 U32 relative
      asave[3] 217..255 u_4 has no such columns: 0 x sigma' = 0
      eaux 39..63, caux 33..63   0
    caux pad rows (npts given): 0 in every column."""
    tag = f"{name}[{layer}]"
    w = valid_width(name, layer)
    if not bool(torch.isfinite(got).all()):
        led.fail(f"{tag} [{case}]: {int((~torch.isfinite(got)).sum())} non-finite words")
        return
    led.add(tag if name in ("act", "asave", "cact") else name, got[:, :w], ref64, ref32, case)
    pad = got[:, w:]
    if name == "act" and layer == 3:
        dev = (pad.double() - SOFTPLUS0).abs().max().item()
        led.expect(dev <= 5.0 * U32 * SOFTPLUS0, f"{tag} [{case}]: pad columns are {dev:.3e} from softplus(0)")
    elif pad.numel():
        led.expect(bool((pad == 0).all()), f"{tag} [{case}]: {int((pad != 0).sum())} non-zero pad-column words")
    if name == "caux" and npts is not None:
        led.expect(bool((got[npts:] == 0).all()), f"{tag} [{case}]: non-zero words in the pad rows")


# ------------------------------------------------------------------------------------------------ tiles of a canary workspace
def region_rows(lay, ws, name, layer=0):
    """[ntiles * 64, 256 or 64] rows of one layer of a tile region of the fp32 workspace `ws`"""
    t = lay.tiles(ws, name, layer)
    return aux_native_to_rows(t) if region_width(name) == 64 else native_to_rows(t)


def write_region_rows(lay, ws, name, layer, rows):
    lay.tiles(ws, name, layer).copy_(aux_rows_to_native(rows) if region_width(name) == 64 else rows_to_native(rows))


def region_range(lay, name):
    return lay.off[name], lay.off[name] + lay.size[name]


def absmax_word(lay, ws, cls):
    return int(ws.view(torch.int32)[lay.absmax + cls * ABSMAX_STRIDE].item()) & 0xFFFFFFFF


def check_canary(led, case, ws_bits, before_bits, owned):
    """ws_bits / before_bits: int32 views of the whole allocation (guards included) after and before the launch; owned: [(start,
    stop)] word ranges the stage must have written.  Every owned word is written (no canary left) and finite; every other word still
    holds what it held before the launch."""
    mask = torch.zeros(ws_bits.numel(), dtype=torch.bool, device=ws_bits.device)
    for a, b in owned:
        mask[a:b] = True
        seg = ws_bits[a:b]
        stale = int((seg == CANARY_BITS).sum())
        led.expect(stale == 0, f"{case}: {stale} words of the owned range [{a}, {b}) were never written")
        led.expect(bool(torch.isfinite(seg.view(F32)).all()), f"{case}: non-finite words in the owned range [{a}, {b})")
    changed = (ws_bits != before_bits) & ~mask
    n = int(changed.sum())
    led.expect(n == 0, f"{case}: {n} words outside the stage's regions were written"
               + (f" (first at word {int(changed.nonzero()[0])})" if n else ""))
