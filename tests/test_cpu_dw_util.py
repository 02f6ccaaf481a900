"""CPU: the restatements in tests/dw_util.py that tests/test_gpu_dw_stage.py relies on, each anchored to the library or to an
independent statement of the same thing -- the workspace carving against dh_workspace_floats, the native tile layouts against the
loop form of tests/test_gpu_saved_tiles.py, the slab order against a transcription of dw.hip slab_elem, the fold against a direct
fp64 autograd."""
import math

import pytest
import torch

from tests import dw_util as U


@pytest.mark.parametrize("npts", [0, 1, 64, 65, 4099, 128 * 2048])
def test_restated_workspace_totals_equal_the_librarys(npts):
    from dynhor_amd import _lib
    lay = U.Layout(npts)
    assert (lay.infer_floats, lay.fwd_floats, lay.total_floats) == _lib.workspace_floats(npts)
    assert lay.ntiles == (npts + 63) // 64
    # regions are contiguous, in carve_workspace's order, and 16-byte aligned
    names = list(lay.off)
    assert names == ["absmax", "tmax", "act", "eaux", "feat", "asave", "cact", "caux", "featbar", "tsave", "t0aux", "rsave", "zbar",
                     "czbar", "tpart", "tred", "slabs", "gesave"]
    o = 0
    for n in names:
        assert lay.off[n] == o and o % 4 == 0, n
        o += lay.size[n]
    assert o == lay.total_floats


def test_slab_geometry():
    assert U.GSTRIDE == 8 * 1024 * sum(U.DW_NBS) == 835584
    assert U.JOB_OFF[0] == 0 and all(U.JOB_OFF[j + 1] == U.JOB_OFF[j] + 8 * U.DW_NBS[j] * 1024 for j in range(14))
    lay = U.Layout(130)
    assert lay.size["slabs"] == (U.DW_G + 1) * U.GSTRIDE and lay.red == lay.slabs + U.DW_G * U.GSTRIDE
    assert lay.red + U.GSTRIDE == lay.gesave


@pytest.mark.parametrize("npts", [64, 129, 1000])
def test_act_offset_equals_the_saved_tile_tests(npts):
    from tests import test_gpu_saved_tiles as S
    nt = (npts + S.TM - 1) // S.TM
    assert U.Layout(npts).act == S.ABSMAX_FLOATS + (S.TMAX_N * nt + 3) // 4 * 4
    assert (U.TILE_F, U.TM) == (S.TILE_F, S.TM)


def test_native_to_rows_agrees_with_the_saved_tile_tests_loop_form():
    from tests.test_gpu_saved_tiles import _native_to_rows
    nt = 3
    t = torch.arange(nt * U.TILE_F, dtype=torch.float32)
    assert torch.equal(U.native_to_rows(t), _native_to_rows(t, nt))


def test_main_tile_pack_unpack_round_trip_and_index():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3 * 64, 256, generator=g)
    n = U.rows_to_native(x)
    assert n.shape == (3 * U.TILE_F,)
    assert torch.equal(U.native_to_rows(n), x)
    assert torch.equal(U.rows_to_native(U.native_to_rows(n)), n)
    # the float4 index of csrc/tile.h, element by element on a few thousand random places
    idx = torch.randint(0, n.numel(), (4096,), generator=g)
    for e in idx.tolist():
        rr, f4 = e % 4, e // 4
        lane, f4 = f4 % 64, f4 // 64
        r4, f4 = f4 % 4, f4 // 4
        t, f4 = f4 % 2, f4 // 2
        m, f4 = f4 % 2, f4 // 2
        w, tile = f4 % 4, f4 // 4
        assert n[e] == x[tile * 64 + 32 * m + 8 * r4 + 4 * (lane >> 5) + rr, 64 * w + 32 * t + (lane & 31)]


def test_aux_tile_pack_unpack_round_trip_and_index():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3 * 64, 64, generator=g)
    n = U.aux_rows_to_native(x)
    assert n.shape == (3 * U.AUXT_F,)
    assert torch.equal(U.aux_native_to_rows(n), x)
    assert torch.equal(U.aux_rows_to_native(U.aux_native_to_rows(n)), n)
    # float4 index ((m*2 + nt)*4 + r4)*64 + lane, as dw.hip's issue / load form it
    for e in torch.randint(0, n.numel(), (4096,), generator=g).tolist():
        rr, f4 = e % 4, e // 4
        lane, f4 = f4 % 64, f4 // 64
        r4, f4 = f4 % 4, f4 // 4
        t, f4 = f4 % 2, f4 // 2
        m, tile = f4 % 2, f4 // 2
        assert n[e] == x[tile * 64 + 32 * m + 8 * r4 + 4 * (lane >> 5) + rr, 32 * t + (lane & 31)]


def _slab_elem_index(nb, o, i):
    """dw.hip slab_elem's index, transcribed"""
    w, ro, j = o >> 5, o & 31, i >> 5
    r = (ro & 3) + 4 * (ro >> 3)
    lane = (i & 31) + 32 * ((ro >> 2) & 1)
    return (w * nb + j) * 1024 + r * 64 + lane


@pytest.mark.parametrize("nb", [2, 8])
def test_slab_to_matrix_inverts_slab_elem(nb):
    slab = torch.arange(8 * nb * 1024, dtype=torch.float64)
    M = U.slab_to_matrix(slab, nb)
    assert M.shape == (256, nb * 32)
    want = torch.tensor([[_slab_elem_index(nb, o, i) for i in range(nb * 32)] for o in range(256)], dtype=torch.float64)
    assert torch.equal(M, want)


def test_job_table_shape():
    assert len(U.JOBS) == 15 and [J["nb"] for J in U.JOBS] == U.DW_NBS
    for j, J in enumerate(U.JOBS):
        for a, b in J["pairs"]:
            assert U.region_width(a[0]) == 256 and U.region_width(b[0]) == 32 * J["nb"], j
            assert 0 <= a[1] < U.REGION_SHAPE[a[0]][0] and 0 <= b[1] < U.REGION_SHAPE[b[0]][0], j
        # every pair has exactly one heavy-tailed operand (the one scaled tile by tile), and its absmax class is a real one
        for ca, ha, cb, hb in U.JOB_CLASSES[j]:
            assert (ha >= 0) != (hb >= 0), j
            assert (ca if ha >= 0 else cb) >= 0, j
    # the two-pair jobs are the SDF layers 0..7 and the skip job
    assert [j for j, J in enumerate(U.JOBS) if len(J["pairs"]) == 2] == list(range(9))
    # classes are distinct words of their tables
    assert len(set(U.ABSMAX.values())) == len(U.ABSMAX) and max(U.ABSMAX.values()) < 64
    assert max(U.TMAX.values()) < U.TMAX_N


def test_scale_words_are_the_bits_of_the_maxima():
    lay = U.Layout(128)
    g = torch.Generator().manual_seed(3)
    ws = torch.randn(lay.tred, generator=g)
    lay.tiles(ws, "zbar", 2)[U.TILE_F + 5] = -77.5
    lay.tiles(ws, "act", 6)[9] = 41.0
    U.write_scale_words(lay, ws)
    wi = ws.view(torch.int32)
    f = lambda v: int(torch.tensor([v], dtype=torch.float32).view(torch.int32).item())
    assert wi[lay.absmax + (U.ABSMAX["zbar"] + 2) * 64] == f(77.5)
    assert wi[lay.absmax + U.ABSMAX["act"] * 64] == f(41.0)
    assert wi[lay.absmax + U.ABSMAX["tag"] * 64] == U.ABSMAX_TAG_F16
    assert wi[lay.tmax + (U.TMAX["zbar"] + 2) * 2 + 1] == f(77.5)
    t0 = lay.tiles(ws, "zbar", 2)[:U.TILE_F].abs().max()
    assert wi[lay.tmax + (U.TMAX["zbar"] + 2) * 2 + 0] == f(float(t0))


def test_fold_reference_equals_a_direct_autograd_of_sum_W_dW():
    from dynhor_amd import _lib
    n_params = int(_lib.lib().dh_num_params())
    g = torch.Generator().manual_seed(4)
    params = torch.randn(n_params, generator=g, dtype=torch.float64)
    jobs = [torch.randint(-4, 5, (256, 32 * nb), generator=g).double() for nb in U.DW_NBS]
    tsum = torch.randint(-4, 5, (20, 256), generator=g).double()
    got = U.fold_reference(jobs, tsum, params)
    assert got.shape == (n_params,)
    var = U.variance_offset()
    assert math.isnan(got[var]) and int(torch.isnan(got).sum()) == 1

    # the same thing written out by hand, one linear after the other: dL/dW gathered element by element as dw.hip fold_kernel
    # gathers it, and L = sum(W * dL/dW) + sum(b * dL/db) differentiated in one piece
    p = params.clone().requires_grad_(True)
    s = 1.0 / math.sqrt(2.0)
    L = 0.0
    for net, n, dims in ((0, 9, U.SDF_DIMS), (2, 5, U.COL_DIMS)):
        for l in range(n):
            b, go, vo, od, idim = _lib.param_layout(net, l)
            assert (od, idim) == dims[l]
            dW = torch.zeros(od, idim, dtype=torch.float64)
            db = torch.zeros(od, dtype=torch.float64)
            for o in range(od):
                if net == 0 and l == 8:
                    dW[o] = tsum[9] + tsum[10] if o == 0 else jobs[9][o - 1]
                    db[o] = tsum[11][0] if o == 0 else tsum[8][o - 1]
                elif net == 0 and l == 4:
                    dW[o, :217] = s * jobs[4][o, :217]
                    dW[o, 217:] = s * jobs[8][o, :39]
                    db[o] = tsum[4][o]
                elif net == 0:
                    dW[o] = jobs[l][o, :idim]
                    db[o] = tsum[l][o]
                elif l == 0:
                    dW[o, :33] = jobs[11][o, :33]
                    dW[o, 33:] = jobs[10][o]
                    db[o] = tsum[12][o]
                elif l == 4:
                    dW[o] = tsum[16 + o]
                    db[o] = tsum[19][o]
                else:
                    dW[o] = jobs[11 + l][o]
                    db[o] = tsum[12 + l][o]
            v = p[vo: vo + od * idim].view(od, idim)
            W = p[go: go + od].view(od, 1) * v / v.pow(2).sum(1, keepdim=True).sqrt()
            L = L + (W * dW).sum() + (p[b: b + od] * db).sum()
    L.backward()
    want = p.grad
    keep = torch.ones(n_params, dtype=torch.bool)
    keep[var] = False
    assert want[var] == 0
    err = (got[keep] - want[keep]).abs().max().item()
    assert err <= 1e-12 * want[keep].abs().max().item(), err
    # lin3 has exactly 217 output rows
    assert [t for t in U.param_tensors() if t[0] == "sdf.lin3.weight_v"][0][2] == (217, 256)


def test_fold_reference_in_fp32_is_close_but_not_identical():
    """the yardstick of the GPU fold test is this function evaluated in fp32"""
    from dynhor_amd import _lib
    n_params = int(_lib.lib().dh_num_params())
    g = torch.Generator().manual_seed(5)
    params = torch.randn(n_params, generator=g)
    jobs = [torch.randint(-8, 9, (256, 32 * nb), generator=g).double() for nb in U.DW_NBS]
    tsum = torch.randint(-8, 9, (20, 256), generator=g).double()
    g64 = U.fold_reference(jobs, tsum, params)
    g32 = U.fold_reference(jobs, tsum, params, dtype=torch.float32)
    assert g32.dtype == torch.float32
    keep = ~torch.isnan(g64)
    rel = (g32.double()[keep] - g64[keep]).abs().max() / g64[keep].abs().max()
    assert 0 < rel < 1e-5
