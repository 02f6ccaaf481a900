"""GPU: the range watch of the two-piece fp16 arithmetic (include/dynhor_hip.h dh_range_words) against fp64 oracles, in both chain
forms of the input-gradient stage.

The register-resident SDF forward chain saves each softplus activation as (hi + lo) / 16 of its two fp16 pieces (csrc/chain_t.hip
T_SAVE_MFMA).  Below 4095 that is the activation; at 4095 and above hi is +inf, lo is -inf, and the transposition MFMA turns the
whole m-tile of saved values into NaN.  dh_sdf_gradient(_ex) reads every saved tile and posts their maximum into the workspace word
dh_range_words names: it must be the largest activation where all are finite and +inf where any is not, never a finite survivor
below the limit.  The weight-gradient launch scales the activations by that word, so behind a +inf word it must write NaN.

Activations are planted exactly: row f of lin_L gets weight_g[f] = 0 and bias c (softplus_100(c) = c for c >> 0.2), and column f of
lin_{L+1}.weight_v is zeroed so the value does not spread.  (weight_v's row stays: a zero row makes the weight norm 0/0.)"""
import copy
import math
from types import SimpleNamespace

import pytest
import torch

from tests.test_gpu_saved_tiles import _native_to_rows, _oracle_activations
from tests.util import flat_from_oracle, randomized_models

pytestmark = pytest.mark.gpu

F16, TILE, PAIR = 2, 0x100, 0x200
FORMS = {"tile": TILE, "pair": PAIR}
TM, TILE_F, ABSMAX_FLOATS, TMAX_N = 64, 16384, 4096, 21
INF_BITS = 0x7F800000
# one planted feature per layer: all four waves (64 columns each) and both 32-column halves of a wave; lin3 has 217 valid features
FEATS = (0, 33, 70, 216, 101, 140, 175, 255)
RAGGED = 64 * 7 + 5


def _plant(sdf, L, f, c):
    lin, nxt = getattr(sdf, f"lin{L}"), getattr(sdf, f"lin{L + 1}")
    with torch.no_grad():
        lin.weight_g[f] = 0.0
        lin.bias[f] = c
        nxt.weight_v[:, f] = 0.0


def _points(npts, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(npts, 3, generator=g) * 2 - 1) * 0.9).cuda()


def _run(hiplib, sdf, col, var, pts, form, fill=0.0):
    """dh_sdf_forward_ex(F16) -> dh_sdf_gradient_ex(F16 | form, save = 1) on a workspace filled with `fill`: (ws, sdf, normals)."""
    from dynhor_amd import _lib
    p = _lib.ptr
    npts = pts.shape[0]
    packed = torch.empty(hiplib.dh_packed_floats(), device=pts.device)
    _lib.check(hiplib.dh_pack_weights(p(flat_from_oracle(sdf, var, col)), p(packed), _lib.stream()))
    ws = torch.full((_lib.workspace_floats(npts)[1],), fill, device=pts.device)
    out = torch.full((npts,), 7.0, device=pts.device)
    normals = torch.full((npts, 3), 7.0, device=pts.device)
    _lib.check(hiplib.dh_sdf_forward_ex(F16, p(packed), p(pts), npts, p(ws), p(out), _lib.stream()))
    _lib.check(hiplib.dh_sdf_gradient_ex(F16 | form, p(packed), p(pts), npts, p(ws), p(normals), 1, _lib.stream()))
    torch.cuda.synchronize()
    return ws, out, normals


def _posted(ws):
    from dynhor_amd import _lib
    a, _, lim = _lib.range_words()
    return float(ws[a]), int(ws[a: a + 1].view(torch.int32).item()) & 0xFFFFFFFF, lim


_RENDERER = []


def _check_range(ws):
    """NeuSRenderer.check_range on a workspace written through the C ABI."""
    from dynhor_amd import _lib
    if not _RENDERER:
        from tests.test_gpu_render_forward import make_pair
        _RENDERER.append(make_pair(seed=5, n_samples=8, n_importance=8)[1])
    return _RENDERER[0].check_range(SimpleNamespace(ws=ws, arith=_lib.ARITH_SPLIT_F16))


def _oracle(sdf, pts):
    """fp64 (sdf [n], normals [n, 3]) of the oracle network."""
    net = copy.deepcopy(sdf).double()
    x = pts.double()
    with torch.no_grad():
        s = net.sdf(x).reshape(-1)
    n = net.gradient(x.clone()).squeeze(1).detach()
    return s, n


def _oracle_act_max(sdf, pts):
    """largest fp64 activation over the 8 layers at the points the saved tiles hold: the real ones, then the ragged tile's pad rows
    (the forward evaluates those at the origin), and softplus(0) in lin3's pad columns."""
    n = pts.shape[0]
    padded = torch.cat([pts, pts.new_zeros((-n) % TM, 3)])
    with torch.no_grad():
        acts = _oracle_activations(copy.deepcopy(sdf), padded)
    return max(max(a.max().item() for a in acts), math.log(2.0) / 100.0)


def _saved_acts(ws, npts):
    nt = (npts + TM - 1) // TM
    act0 = ABSMAX_FLOATS + (TMAX_N * nt + 3) // 4 * 4                       # csrc/workspace.h carve_workspace
    return [_native_to_rows(ws[act0 + l * nt * TILE_F: act0 + (l + 1) * nt * TILE_F], nt) for l in range(8)]


# ------------------------------------------------------------------------------------------------ 1. which activation is reported
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", range(8))
def test_posted_word_is_the_fp64_maximum_on_every_read_path(hiplib, L, form):
    """act[7] is read by acc_load_native_b, act[0..6] by the two slabs of the layer loop (TILE) / the epilogue ring (PAIR)."""
    sdf, col, var = randomized_models(seed=41, device="cuda:0", jitter=0.05)
    c = 3000.0 + 1.25 * L
    _plant(sdf, L, FEATS[L], c)
    pts = _points(RAGGED, seed=L)
    ws, _, _ = _run(hiplib, sdf, col, var, pts, FORMS[form])
    m, _, lim = _posted(ws)
    ref = _oracle_act_max(sdf, pts)
    print(f"L={L} f={FEATS[L]} {form}: posted {m!r}, fp64 maximum {ref!r}")
    assert ref == c
    assert abs(m - ref) <= 1e-5 * ref
    assert _check_range(ws) == (m, lim)


# ------------------------------------------------------------------------------------------------ 2. the edges of the limit
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", [0, 3, 7])
def test_the_finite_band_above_the_limit_is_reported_and_still_valid(hiplib, L, form):
    from dynhor_amd import _lib
    sdf, col, var = randomized_models(seed=43, device="cuda:0", jitter=0.05)
    c = 4094.5                                                               # 16 c = 65512 rounds to fp16 65504: finite
    _plant(sdf, L, FEATS[L], c)
    pts = _points(RAGGED, seed=100 + L)
    ws, s, n = _run(hiplib, sdf, col, var, pts, FORMS[form])
    m, bits, lim = _posted(ws)
    s64, n64 = _oracle(sdf, pts)
    es, en = (s.double() - s64).abs().max().item(), (n.double() - n64).abs().max().item()
    print(f"L={L} {form}: posted {m!r} (limit {lim}); |sdf - fp64| {es:.2e}, |normal - fp64| {en:.2e}")
    assert math.isfinite(m) and abs(m - c) <= 1e-5 * c and m > lim
    with pytest.raises(_lib.DynhorHipError, match="split_f16 range exceeded"):
        _check_range(ws)
    assert es < 2e-5 and en < 2e-4


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", [0, 3, 7])
def test_an_activation_of_4096_at_every_point_posts_inf(hiplib, L, form):
    from dynhor_amd import _lib
    sdf, col, var = randomized_models(seed=43, device="cuda:0", jitter=0.05)
    _plant(sdf, L, FEATS[L], 4096.0)
    ws, s, _ = _run(hiplib, sdf, col, var, _points(RAGGED, seed=200 + L), FORMS[form])
    m, bits, _ = _posted(ws)
    print(f"L={L} {form}: posted {m!r} (bits {bits:#010x}); finite sdf {int(torch.isfinite(s).sum())} of {s.numel()}")
    assert bits == INF_BITS
    with pytest.raises(_lib.DynhorHipError, match="split_f16 range exceeded"):
        _check_range(ws)


# ------------------------------------------------------------------------------------------------ 3. one overflowing point
def _one_point_net(seed, npts, hot):
    """lin0 feature 5 = 10 x + b with b such that the point `hot` (x = 0.99) reaches 4095.5 (16 x 4095.5 overflows fp16) and every
    other point (|x| <= 0.9) stays below 4094.6: finite, above the limit."""
    sdf, col, var = randomized_models(seed=seed, device="cuda:0", jitter=0.05)
    f = 5
    with torch.no_grad():
        sdf.lin0.weight_v[f] = 0.0
        sdf.lin0.weight_v[f, 0] = 1.0                                        # embedding column 0 = x (net.scale 1)
        sdf.lin0.weight_g[f] = 10.0
        sdf.lin0.bias[f] = 4095.5 - 10.0 * 0.99
        sdf.lin1.weight_v[:, f] = 0.0
    pts = _points(npts, seed=seed)
    pts[hot, 0] = 0.99
    return sdf, col, var, pts


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("hot", [0, RAGGED - 1], ids=["point0_tile0", "last_point_ragged_tile"])
def test_one_overflowing_point_posts_inf_and_the_finite_results_stay_valid(hiplib, hot, form):
    sdf, col, var, pts = _one_point_net(47, RAGGED, hot)
    ws, s, n = _run(hiplib, sdf, col, var, pts, FORMS[form])
    m, bits, _ = _posted(ws)
    s64, n64 = _oracle(sdf, pts)
    assert torch.isfinite(s64).all()
    fs, fn = torch.isfinite(s), torch.isfinite(n).all(1)
    tile = torch.arange(RAGGED, device=s.device) // TM == hot // TM
    es = (s.double() - s64)[fs].abs().max().item()
    en = (n.double() - n64)[fn].abs().max().item()
    print(f"hot point {hot} ({form}): posted {m!r} (bits {bits:#010x}); non-finite sdf {int((~fs).sum())}, non-finite normals "
          f"{int((~fn).sum())} (in the hot tile: {int((~fn & tile).sum())} of {int(tile.sum())}, elsewhere: {int((~fn & ~tile).sum())}); "
          f"finite |sdf - fp64| {es:.2e}, |normal - fp64| {en:.2e}")
    assert bits == INF_BITS
    assert not bool(fs[hot]) and int((~fs).sum()) == 1
    assert not bool((~fn & ~tile).any()), "a non-finite normal outside the overflowing point's tile"
    assert es < 2e-5 and en < 2e-4


# ------------------------------------------------------------------------------------------------ 4. unwritten words are not read
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("fill", [1e30, float("nan")], ids=["1e30", "nan"])
@pytest.mark.parametrize("npts", [RAGGED, 64 * 6 + 5, 64 * 5 + 63])
def test_the_watch_reads_only_what_the_forward_wrote(hiplib, npts, fill, form):
    sdf, col, var = randomized_models(seed=53, device="cuda:0", jitter=0.05)
    pts = _points(npts, seed=npts)
    ws, s, n = _run(hiplib, sdf, col, var, pts, FORMS[form], fill=fill)
    m, _, lim = _posted(ws)
    ref = _oracle_act_max(sdf, pts)
    print(f"npts={npts} fill={fill} {form}: posted {m!r}, fp64 maximum {ref!r}")
    assert torch.isfinite(s).all() and torch.isfinite(n).all()
    assert abs(m - ref) <= 1e-5 * ref and m < lim


def test_saved_activation_tiles_never_carry_the_sign_bit_at_zero(hiplib):
    """The watch maximum is taken over fp32 bit patterns (csrc/tile16h.h watch_max3): a saved activation of exactly zero must be +0.
    softplus_100 underflows to 0 below about -1.04: planted biases drive one feature per layer there."""
    sdf, col, var = randomized_models(seed=57, device="cuda:0", jitter=0.05)
    for L in range(8):
        _plant(sdf, L, FEATS[L], -50.0)
    npts = RAGGED
    ws, _, _ = _run(hiplib, sdf, col, var, _points(npts, seed=3), TILE)
    acts = _saved_acts(ws, npts)
    for L in range(8):
        col_ = acts[L][:, FEATS[L]]
        assert bool((col_ == 0).all()), (L, col_.abs().max().item())
        assert not bool((acts[L].view(torch.int32) < 0).any()), L


# ------------------------------------------------------------------------------------------------ 5. every point overflows
def _overflow_pair(seed=35):
    from tests.test_gpu_range_safety import _scaled_pair
    def scale(sdf, col):
        sdf.lin1.weight_g *= 3.0e6
    return _scaled_pair(scale, seed=seed)


def _segments(sdf):
    """{state_dict name: (offset, shape)} of the SDF network in the flat parameter (and gradient) vector."""
    out, off = {}, 0
    for k, v in sdf.state_dict().items():
        out[k] = (off, tuple(v.shape))
        off += v.numel()
    return out


def test_every_overflow_posts_inf_and_poisons_the_weight_gradients():
    from dynhor_amd import _lib
    from tests.test_gpu_render_forward import make_pair, make_rays
    o_r, p_r = _overflow_pair()
    o, d, near, far, t_rand = make_rays(64, seed=5)
    z = o_r.sample_z(o, d, near, far, t_rand=t_rand)
    s = p_r._forward_core(o, d, z, 0.5, None, want_nmap=False)
    torch.cuda.synchronize()
    m, bits, lim = _posted(s.ws)
    print(f"forward: posted {m!r} (bits {bits:#010x})")
    assert bits == INF_BITS
    with pytest.raises(_lib.DynhorHipError, match="split_f16 range exceeded"):
        p_r.check_range(s)

    rays = torch.cat([o, d, torch.rand(64, 3, device="cuda:0"), torch.ones(64, 2, device="cuda:0"), torch.zeros(64, 3, device="cuda:0")], -1).contiguous()
    p_r.train_step_core(rays, near, far, None, 0.5, 0.1, 0.1, 0.0, t_rand=t_rand)
    torch.cuda.synchronize()
    st = p_r.last_state
    m, bits, lim = _posted(st.ws)
    assert bits == INF_BITS
    with pytest.raises(_lib.DynhorHipError, match="split_f16 range exceeded"):
        p_r.check_range(st)
    grad = p_r.store.grad_flat
    seg = _segments(o_r.sdf_network)
    # weight-gradient jobs 1..7 (lin1..lin7: act[l-1] is their B operand) and 9 (lin8's feature rows 1..256: act[7])
    parts = {f"lin{l}.{w}": grad[seg[f"lin{l}.{w}"][0]: seg[f"lin{l}.{w}"][0] + math.prod(seg[f"lin{l}.{w}"][1])].view(seg[f"lin{l}.{w}"][1])
             for l in range(1, 9) for w in ("weight_v", "weight_g")}
    for name, g in parts.items():
        if name.startswith("lin8"):
            g = g[1:]
        finite = int(torch.isfinite(g).sum())
        assert finite == 0 and bool(torch.isnan(g).all()), f"{name}: {finite} finite of {g.numel()}"

    # a normal step on the same workspace: the stored +inf does not persist
    _, normal = make_pair(seed=35, n_samples=32, n_importance=32)
    ws_before = st.ws.data_ptr()
    p_r.sdf_network.load_state_dict(normal.sdf_network.state_dict())
    p_r.train_step_core(rays, near, far, None, 0.5, 0.1, 0.1, 0.0, t_rand=t_rand)
    torch.cuda.synchronize()
    st2 = p_r.last_state
    m2, _, _ = _posted(st2.ws)
    print(f"normal step: posted {m2!r} (same workspace: {st2.ws.data_ptr() == ws_before})")
    assert 0.0 < m2 < lim and torch.isfinite(p_r.store.grad_flat).all()
    assert p_r.check_range(st2) == (m2, lim)


# ------------------------------------------------------------------------------------------------ 7. the no-grad chain, bf16
def _nograd(hiplib, arith, sdf, col, var, pts):
    from dynhor_amd import _lib
    p = _lib.ptr
    packed = torch.empty(hiplib.dh_packed_floats(), device=pts.device)
    _lib.check(hiplib.dh_pack_weights(p(flat_from_oracle(sdf, var, col)), p(packed), _lib.stream()))
    out = torch.full((pts.shape[0],), 7.0, device=pts.device)
    _lib.check(hiplib.dh_sdf_nograd_ex(arith, p(packed), p(pts), pts.shape[0], p(out), _lib.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("hot", [0, RAGGED - 1], ids=["point0", "last_point"])
def test_nograd_chain_one_overflowing_point(hiplib, hot):
    sdf, col, var, pts = _one_point_net(47, RAGGED, hot)
    out = _nograd(hiplib, F16, sdf, col, var, pts)
    s64, _ = _oracle(sdf, pts)
    fin = torch.isfinite(out)
    err = (out.double() - s64)[fin].abs().max().item()
    print(f"no-grad, hot point {hot}: non-finite {int((~fin).sum())}; finite |sdf - fp64| {err:.2e}")
    assert not bool(fin[hot]) and int((~fin).sum()) == 1
    assert err < 2e-5


def test_nograd_chain_every_overflow_and_extract_geometry_raise(hiplib):
    from dynhor_amd import _lib
    o_r, p_r = _overflow_pair()
    sdf, col, var = o_r.sdf_network, o_r.color_network, o_r.deviation_network
    pts = _points(RAGGED, seed=9)
    out = _nograd(hiplib, F16, sdf, col, var, pts)
    print(f"no-grad, every overflow: finite {int(torch.isfinite(out).sum())} of {out.numel()}")
    assert not torch.isfinite(out).any()
    with pytest.raises(_lib.DynhorHipError):
        p_r.extract_geometry([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], 32)

    # the three-piece bf16 arithmetic has no such limit: the sdf matches fp64 as closely as torch's own fp32 does
    out_bf = _nograd(hiplib, _lib.ARITH_SPLIT_BF16, sdf, col, var, pts)
    s64, _ = _oracle(sdf, pts)
    with torch.no_grad():
        s32 = copy.deepcopy(sdf).float().sdf(pts).reshape(-1)
    e_hip = (out_bf.double() - s64).abs().max().item()
    e_t32 = (s32.double() - s64).abs().max().item()
    print(f"split_bf16 on the overflow network: max |sdf| {s64.abs().max().item():.3g}; |hip - fp64| {e_hip:.3e}, "
          f"|torch fp32 - fp64| {e_t32:.3e} (ratio {e_hip / e_t32:.2f})")
    assert torch.isfinite(out_bf).all()
    assert e_hip <= 10 * e_t32
