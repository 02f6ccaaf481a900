"""The hash-grid family's geometry kernels bit for bit against tests/golden/hash_kernel_bits.json: one SHA-256 per output buffer of
dh_hash_sdf_nograd, dh_hash_geo_forward (sdf, feature, gradient, workspace), dh_hash_geo_backward (workspace),
dh_hash_geo_backward_rays (workspace, d_pts) and dh_hash_weight_grads_parts with parts 7 (the reproducible scatter: the whole gradient
vector), called through the C ABI and recorded by tests/golden/make_golden_hash_kernel_bits.py at the commit the file names.  Every one
of these outputs is reproducible by construction (no float atomics: the table scatter runs in its fixed-point form), so a change to
hash_mlp.hip or hashgrid_dev.h that means to change no arithmetic must leave every hash as it is: a differing hash is a finding to
explain, never a reason to record again.

Every output buffer is filled with one NaN bit pattern (SENTINEL) before the call and hashed whole, so rows past n_active and the
padding of the feature-major workspace rows are held to stay untouched.  The workspace is hashed as (length, positions that differ from
the sentinel, bits there) and the gradient vector as the same against zero -- that determines the buffer exactly and costs what was
written, not the 130 MB a workspace spans; the workspace's tail (the fixed-point accumulators, 2 x (entries x 2 + 8) floats,
include/dynhor_hip.h) is only the scatter's, so after the forward and the two backwards it is asserted to be all sentinel and left out
of the hash.  Inputs are hashed too ("in:" entries): a failure says whether the inputs or a kernel moved.

Sizes: n = 1, 63, 65, 255, 257, 1000 (across the scatter's 64-point block and the 256-thread workgroup), capacity 1000 with n_active
700, and with n_active 0.  Points (radius 1, eps 1e-3, numpy RandomState(SEED)), 44 to a chunk so that the first 63 hold every kind:
  8 uniform in the box; 8 within eps/2 of a cell face of levels 12..15, every axis and side in turn (the shifted evaluation lands in the
  neighbour cell: the four outer corners are gathered again); a run of 16 consecutive samples 2e-3 apart (one coarse cell: the scatter's
  lane runs have something to merge); 4 on a face to fp32; 4 on the box's far faces (a dense level's corner coordinate reaches res);
  4 outside the box, either side (the negative floor wraps in uint32)."""
import ctypes
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_kernel_bits.json")
SEED = 20261
RADIUS, EPS = 1.0, 1e-3
SENTINEL = 0x7FC0DEAD                                # a quiet NaN no kernel writes
POOL = 1000
# case -> (capacity n, n_active or None)
CASES = {"n1": (1, None), "n63": (63, None), "n65": (65, None), "n255": (255, None), "n257": (257, None), "n1000": (1000, None),
         "packed_700_of_1000": (1000, 700), "packed_0_of_1000": (1000, 0)}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def sha_sparse(t, fill):
    """SHA-256 of (length, positions whose bits differ from `fill`, the bits there): one to one with the whole buffer."""
    bits = t.detach().contiguous().view(-1).view(torch.int32)
    idx = (bits != fill).nonzero().view(-1)
    h = hashlib.sha256(str(bits.numel()).encode())
    h.update(idx.cpu().numpy().tobytes())
    h.update(bits[idx].cpu().numpy().tobytes())
    return h.hexdigest()


def level_scales():
    """hashgrid_dev.h make_levels(): scale_l = 16 (2048 / 16)^(l / 15) - 1."""
    pls = math.exp((math.log(2048.0) - math.log(16.0)) / 15)
    return [16 * pls ** l - 1.0 for l in range(16)]


@functools.lru_cache(maxsize=None)
def points():
    """[POOL, 3] fp32 on the CPU, as the module's docstring lays them out."""
    rs, S, out, k = np.random.RandomState(SEED), level_scales(), [], 0
    face = lambda l: 2.0 * (rs.randint(1, int(S[l])) - 0.5) / S[l] - 1.0              # a cell face of level l, world units
    for chunk in range((POOL + 43) // 44):
        out.append(rs.uniform(-1, 1, (8, 3)))
        near = rs.uniform(-1, 1, (8, 3))
        for j in range(8):
            l, a, side = 12 + k % 4, (k // 4) % 3, 1.0 if (k // 12) % 2 else -1.0
            near[j, a] = face(l) + side * rs.uniform(0, EPS / 2)
            k += 1
        out.append(near)
        d = rs.randn(3)
        out.append(rs.uniform(-0.9, 0.9, 3)[None] + (np.arange(16) * 2e-3)[:, None] * (d / np.linalg.norm(d))[None])
        on = rs.uniform(-1, 1, (4, 3))
        for j in range(4):
            on[j, (chunk + j) % 3] = np.float32(face(12 + j))
        out.append(on)
        far = rs.uniform(-1, 1, (4, 3))
        far[0, chunk % 3] = far[1, (chunk + 1) % 3] = 1.0
        far[2, [chunk % 3, (chunk + 1) % 3]] = 1.0
        far[3, :] = 1.0
        out.append(far)
        outside = rs.uniform(-1, 1, (4, 3))
        for j in range(4):
            outside[j, (chunk + j) % 3] = (1.0 if j & 1 else -1.0) * rs.uniform(1.0005, 1.5)
        out.append(outside)
    return torch.from_numpy(np.concatenate(out)[:POOL].astype(np.float32)).contiguous()


@functools.lru_cache(maxsize=None)
def cotangents():
    """(d_sdf [POOL], d_feature [POOL, 13], d_normals [POOL, 3]) on the CPU, small enough that no merged contribution of the fixed-point
    scatter nears its limit of 64 (the +-0.5 / eps on the finite-difference rows included), and the colour network's filler inputs
    (feature, normals, dirs, d_color): dh_hash_color_backward fills the colour rows that parts 7 reads."""
    rs = np.random.RandomState(SEED + 1)
    f = lambda a: torch.from_numpy(a.astype(np.float32)).contiguous()
    d = rs.randn(POOL, 3)
    return {"d_sdf": f(0.05 * rs.randn(POOL)), "d_feature": f(0.05 * rs.randn(POOL, 13)), "d_normals": f(5e-5 * rs.randn(POOL, 3)),
            "c_feature": f(rs.randn(POOL, 13)), "c_normals": f(rs.randn(POOL, 3)), "c_dirs": f(d / np.linalg.norm(d, axis=1, keepdims=True)),
            "c_d_color": f(0.05 * rs.randn(POOL, 3))}


def _layout(L, net, layer):
    b, g, v = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    o, i = ctypes.c_int32(), ctypes.c_int32()
    assert L.dh_hash_param_layout(net, layer, ctypes.byref(b), ctypes.byref(g), ctypes.byref(v), ctypes.byref(o), ctypes.byref(i)) == 0
    return b.value, g.value, v.value, o.value, i.value


@functools.lru_cache(maxsize=None)
def parameters():
    """(params on the device, packed weights, their hashes, table entries): a table of +-0.5 so that every gathered value weighs in the
    sums, weight-norm directions N(0, 0.3), gains in 0.5..1, biases N(0, 0.1)."""
    from dynhor_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(SEED + 2)
    flat = np.zeros(int(L.dh_hash_num_params()), dtype=np.float32)
    _, _, toff, entries, feats = _layout(L, 3, 0)
    flat[toff:toff + entries * feats] = rs.uniform(-0.5, 0.5, entries * feats)
    for net, layers in ((0, 2), (2, 3)):
        for layer in range(layers):
            b, g, v, out_dim, in_dim = _layout(L, net, layer)
            flat[b:b + out_dim] = 0.1 * rs.randn(out_dim)
            flat[g:g + out_dim] = rs.uniform(0.5, 1.0, out_dim)
            flat[v:v + out_dim * in_dim] = 0.3 * rs.randn(out_dim * in_dim)
    flat[_layout(L, 1, 0)[2]] = 0.3
    params = torch.from_numpy(flat).to(DEV)
    packed = sentinel(int(L.dh_hash_packed_floats()))
    _lib.check(L.dh_hash_pack_weights(_p(params), _p(packed), _lib.stream()))
    torch.cuda.synchronize()
    return params, packed, {"in:params": sha(params), "in:packed": sha(packed)}, entries * feats


def hashes(case):
    """{buffer: SHA-256} of one case, inputs included."""
    from dynhor_amd import _lib
    L, st = _lib.lib(), _lib.stream()
    n, act = CASES[case]
    params, packed, out, table_floats = parameters()
    out = dict(out)
    pts = points()[:n].to(DEV).contiguous()
    cot = {k: v[:n].to(DEV).contiguous() for k, v in cotangents().items()}
    n_act = None if act is None else torch.tensor([act], dtype=torch.int64, device=DEV)
    out["in:pts"] = sha(pts)
    out.update({"in:" + k: sha(v) for k, v in cot.items()})
    infer, total = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.dh_hash_workspace_floats(n, ctypes.byref(infer), ctypes.byref(total)))
    head = total.value - 2 * (table_floats + 8)                # the rows and slabs; behind them the scatter's int64 accumulators

    def ws_sha(ws):
        assert bool((ws[head:].view(torch.int32) == SENTINEL).all()), "the accumulators' range was written outside the scatter"
        return sha_sparse(ws[:head], SENTINEL)

    if act is None:
        sdf = sentinel(n)
        _lib.check(L.dh_hash_sdf_nograd(_p(params), _p(packed), _p(pts), n, RADIUS, _p(sdf), st))
        out["sdf_nograd"] = sha(sdf)
    ws = sentinel(total.value)
    sdf, feat, grad = sentinel(n), sentinel(n, 13), sentinel(n, 3)
    _lib.check(L.dh_hash_geo_forward(_p(params), _p(packed), _p(pts), n, RADIUS, EPS, _p(ws), 1, _p(sdf), _p(feat), _p(grad), _p(n_act), st))
    out.update({"forward_sdf": sha(sdf), "forward_feature": sha(feat), "forward_gradient": sha(grad), "forward_ws": ws_sha(ws)})
    geo = (_p(params), _p(packed), _p(pts), _p(cot["d_sdf"]), _p(cot["d_feature"]), _p(cot["d_normals"]), n, RADIUS, EPS)
    plain = ws.clone()
    _lib.check(L.dh_hash_geo_backward(*geo, _p(plain), _p(n_act), st))
    out["backward_ws"] = ws_sha(plain)
    del plain
    d_pts = sentinel(n, 3)
    _lib.check(L.dh_hash_geo_backward_rays(*geo, _p(ws), _p(n_act), _p(d_pts), st))
    out.update({"backward_rays_ws": ws_sha(ws), "backward_rays_d_pts": sha(d_pts)})
    d_feat, d_nrm = sentinel(n, 13), torch.zeros(n, 3, device=DEV)
    _lib.check(L.dh_hash_color_backward(_p(packed), _p(cot["c_feature"]), _p(cot["c_normals"]), _p(cot["c_dirs"]), _p(cot["c_d_color"]), 1,
                                        n, _p(ws), _p(d_feat), _p(d_nrm), _p(n_act), st))
    g = sentinel(params.numel())
    _lib.check(L.dh_hash_weight_grads_parts(_p(params), _p(packed), n, _p(ws), _p(g), _p(n_act), 7, st))
    torch.cuda.synchronize()
    out["weight_grads"] = sha_sparse(g, 0)
    out["weight_grads_finite"] = bool(torch.isfinite(g[:table_floats]).all())       # a NaN table would hide every bit of the scatter
    return out


@functools.lru_cache(maxsize=None)
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_covers_the_cases():
    rec = recorded()["hashes"]
    assert sorted(rec) == sorted(CASES)
    for case, (n, act) in CASES.items():
        assert ("sdf_nograd" in rec[case]) == (act is None), case
        assert {"forward_sdf", "forward_feature", "forward_gradient", "forward_ws", "backward_ws", "backward_rays_ws",
                "backward_rays_d_pts", "weight_grads"} <= set(rec[case]), case
        assert rec[case]["weight_grads_finite"] is True, case
        # the rows the weight gradients read are the same with and without the point adjoint
        assert rec[case]["backward_ws"] == rec[case]["backward_rays_ws"], case
    assert len({rec[c]["weight_grads"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_hash_kernels_match_the_recording_bit_for_bit(case):
    want, got = recorded()["hashes"][case], hashes(case)
    assert sorted(want) == sorted(got), f"{case}: the buffers differ from the recording's"
    moved_in = sorted(k for k in want if k.startswith("in:") and want[k] != got[k])
    assert not moved_in, f"{case}: the INPUTS differ from the recording's: {moved_in}"
    moved = sorted(k for k in want if want[k] != got[k])
    assert not moved, f"{case}: {moved} differ from the recording"
