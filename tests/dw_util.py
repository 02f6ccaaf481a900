"""Plain restatements of what the weight-gradient stage (csrc/dw.hip) reads and writes, for the tests that drive it alone.

Nothing here launches a kernel and everything works on CPU tensors: the workspace carving (csrc/workspace.h carve_workspace), the
split-K slab geometry and job table (dw.hip build_dw_jobs), the native tile layouts (csrc/tile.h, MT = 2), the slab element order
(dw.hip slab_elem) and an fp64 statement of the fold (dw.hip fold_kernel / build_fold_table) that gets (d bias, d g, d v) by torch
autograd through W = g v / |v| instead of the kernel's closed form.  tests/test_cpu_dw_util.py anchors each of them to the library
(dh_workspace_floats, dh_param_layout) or to an independent statement before tests/test_gpu_dw_stage.py relies on them.
"""
import math

import torch

# ---------------------------------------------------------------- csrc/layout.h
TM, HID = 64, 256
TILE_F, AUXT_F = TM * HID, TM * 64
N_SDF, N_COL = 9, 5
EMB, CAUX, SKIP_OUT = 39, 33, 217
SDF_DIMS = [(256, 39), (256, 256), (256, 256), (217, 256), (256, 256), (256, 256), (256, 256), (256, 256), (257, 256)]
COL_DIMS = [(256, 289), (256, 256), (256, 256), (256, 256), (3, 256)]
H2_XS = 16.0

# ---------------------------------------------------------------- csrc/workspace.h
N_TILE_PART, DW_G, DW_NS = 20, 256, 64
ABSMAX_STRIDE = 64
ABSMAX_FLOATS = 64 * ABSMAX_STRIDE
ABSMAX = dict(asave=0, zbar=8, tsave=16, t0aux=23, featbar=24, czbar=25, cact=29, feat=33, act=34, caux=35, tag=36)
ABSMAX_TAG_F16 = 0x00F16F16
TMAX = dict(zbar=0, featbar=8, czbar=9, tsave=13, t0aux=20)
TMAX_N = 21
H2_AT = 8

# region -> (layers, floats per tile and layer), in carve_workspace's order between tmax and tpart
TILE_REGIONS = [("act", 8, TILE_F), ("eaux", 1, AUXT_F), ("feat", 1, TILE_F), ("asave", 8, TILE_F), ("cact", 4, TILE_F),
                ("caux", 1, AUXT_F), ("featbar", 1, TILE_F), ("tsave", 7, TILE_F), ("t0aux", 1, AUXT_F), ("rsave", 8, TILE_F),
                ("zbar", 8, TILE_F), ("czbar", 4, TILE_F)]
REGION_SHAPE = {name: (layers, per) for name, layers, per in TILE_REGIONS}
# the operands whose distribution is heavy-tailed (adjoints and tangents): the ones with a per-tile maximum
HEAVY = ("zbar", "featbar", "czbar", "tsave", "t0aux")
# every region a job reads
OPERAND_REGIONS = ("act", "eaux", "feat", "asave", "cact", "caux", "featbar", "tsave", "t0aux", "zbar", "czbar")

# ---------------------------------------------------------------- dw.hip slab geometry
DW_NBS = [2, 8, 8, 8, 8, 8, 8, 8, 2, 8, 8, 2, 8, 8, 8]
JOB_FLOATS = [8 * nb * 1024 for nb in DW_NBS]
JOB_OFF = [sum(JOB_FLOATS[:j]) for j in range(15)]
GSTRIDE = sum(JOB_FLOATS)


def dw_slab_floats(G=DW_G):
    return (G + 1) * GSTRIDE


class Layout:
    """carve_workspace(npts): float offsets of every region (attributes and .off[name]), .size[name], ntiles and the three totals."""

    def __init__(self, npts):
        nt = (npts + TM - 1) // TM
        self.npts, self.ntiles = npts, nt
        self.off, self.size = {}, {}
        o = 0

        def take(name, n):
            nonlocal o
            self.off[name], self.size[name] = o, n
            setattr(self, name, o)
            o += n
        take("absmax", ABSMAX_FLOATS)
        take("tmax", (TMAX_N * nt + 3) // 4 * 4)
        for name, layers, per in TILE_REGIONS:
            take(name, layers * nt * per)
            if name == "feat":
                self.infer_floats = o
            if name == "caux":
                self.fwd_floats = o
        take("tpart", nt * N_TILE_PART * 256)
        take("tred", DW_NS * N_TILE_PART * 256)
        take("slabs", dw_slab_floats(DW_G))
        take("gesave", nt * TM * 40)
        self.total_floats = o
        self.red = self.slabs + DW_G * GSTRIDE           # the reduced block behind the DW_G split blocks

    def tiles(self, ws, name, layer=0):
        """the [ntiles * floats-per-tile] slice of `ws` holding layer `layer` of a tile region"""
        layers, per = REGION_SHAPE[name]
        assert 0 <= layer < layers
        a = self.off[name] + layer * self.ntiles * per
        return ws[a: a + self.ntiles * per]

    def red_job(self, ws, job):
        a = self.red + JOB_OFF[job]
        return ws[a: a + JOB_FLOATS[job]]


# ---------------------------------------------------------------- native tiles (csrc/tile.h, MT = 2)
# main: float4 index (((w*2 + m)*2 + t)*4 + r4)*64 + lane, element rr <-> row 32 m + 8 r4 + 4 (lane >> 5) + rr, col 64 w + 32 t + (lane & 31)
def rows_to_native(x):
    """[P, 256] (P a multiple of 64) -> [P * 256] native main tiles"""
    P = x.shape[0]
    assert x.shape == (P, 256) and P % TM == 0
    v = x.reshape(P // TM, 2, 4, 2, 4, 4, 2, 32)           # tile | row: m, r4, h, rr | col: w, t, c
    return v.permute(0, 5, 1, 6, 2, 3, 7, 4).reshape(-1)   # tile, w, m, t, r4, (h, c) = lane, rr


def native_to_rows(t):
    """[nt * TILE_F] native main tiles -> [nt * 64, 256]"""
    v = t.reshape(-1, 4, 2, 2, 4, 2, 32, 4)                # tile, w, m, t, r4, h, c, rr
    return v.permute(0, 2, 4, 5, 7, 1, 3, 6).reshape(-1, 256)


# aux: float4 index ((m*2 + t)*4 + r4)*64 + lane, element rr <-> row 32 m + 8 r4 + 4 (lane >> 5) + rr, col 32 t + (lane & 31)
def aux_rows_to_native(x):
    """[P, 64] -> [P * 64] native aux tiles"""
    P = x.shape[0]
    assert x.shape == (P, 64) and P % TM == 0
    v = x.reshape(P // TM, 2, 4, 2, 4, 2, 32)              # tile | row: m, r4, h, rr | col: t, c
    return v.permute(0, 1, 5, 2, 3, 6, 4).reshape(-1)      # tile, m, t, r4, (h, c), rr


def aux_native_to_rows(t):
    v = t.reshape(-1, 2, 2, 4, 2, 32, 4)                   # tile, m, t, r4, h, c, rr
    return v.permute(0, 1, 3, 4, 6, 2, 5).reshape(-1, 64)


def region_to_native(name, x):
    return aux_rows_to_native(x) if REGION_SHAPE[name][1] == AUXT_F else rows_to_native(x)


def region_width(name):
    return 64 if REGION_SHAPE[name][1] == AUXT_F else 256


# ---------------------------------------------------------------- slabs
def slab_to_matrix(red_job, nb):
    """One job's slab [8 * nb * 1024] -> [256, nb * 32]: the inverse of dw.hip slab_elem,
    index ((w*nb + j)*1024 + r*64 + lane) with o = 32 w + 8 (r >> 2) + 4 (lane >> 5) + (r & 3), i = 32 j + (lane & 31)."""
    v = red_job.reshape(8, nb, 4, 4, 2, 32)                # w, j, q = r >> 2, s = r & 3, h, c
    return v.permute(0, 2, 4, 3, 1, 5).reshape(256, nb * 32)


# ---------------------------------------------------------------- the job table (dw.hip build_dw_jobs)
# per job: the operand pairs ((A region, layer), (B region, layer)); B of width 64 is an aux tile.  Output rows = A's columns.
def _job(a1, b1, a2=None, b2=None):
    return dict(pairs=[(a1, b1)] + ([(a2, b2)] if a2 else []))


JOBS = ([_job(("zbar", 0), ("eaux", 0), ("asave", 0), ("t0aux", 0))]
        + [_job(("zbar", l), ("act", l - 1), ("asave", l), ("tsave", l - 1)) for l in range(1, 8)]
        + [_job(("zbar", 4), ("eaux", 0), ("asave", 4), ("t0aux", 0)),
           _job(("featbar", 0), ("act", 7)),
           _job(("czbar", 0), ("feat", 0)),
           _job(("czbar", 0), ("caux", 0))]
        + [_job(("czbar", l), ("cact", l - 1)) for l in range(1, 4)])
for _j, _J in enumerate(JOBS):
    _J["nb"] = DW_NBS[_j]


def absmax_class(name, layer):
    """absmax class of an operand (workspace.h); -1: carried at the constant H2_XS (the embedding tile).  The eight softplus
    activations share ABSMAX_ACT."""
    if name == "eaux":
        return -1
    return ABSMAX[name] + (0 if name == "act" else layer)


def tmax_class(name, layer):
    """tmax class of a heavy-tailed operand, -1 for a tame one"""
    return TMAX[name] + layer if name in TMAX else -1


# the two-piece fp16 form's classes per job and pair: (ca, ha, cb, hb) as build_dw_jobs' C_ sets them
JOB_CLASSES = [[(absmax_class(*a), tmax_class(*a), absmax_class(*b), tmax_class(*b)) for a, b in J["pairs"]] for J in JOBS]


def job_product(job, rows, dtype=torch.float64):
    """sum over the job's pairs of A^T B in `dtype`; rows[(region, layer)] = [P, width] row-form operands"""
    out = None
    for a, b in JOBS[job]["pairs"]:
        p = rows[a].to(dtype).t() @ rows[b].to(dtype)
        out = p if out is None else out + p
    return out


def max_bits(x):
    """the fp32 bits of max |x| as a 0-dim int32 tensor on x's device (what the absmax / tmax words hold)"""
    return x.abs().max().float().reshape(1).view(torch.int32)[0]


def scale_words(lay, ws):
    """(absmax words {class: bits}, tmax words int32 [TMAX_N, ntiles]) of the operand tiles in `ws`, as workspace.h defines them: each
    word is the fp32 bits of the maximum |value|; ABSMAX_ACT covers all eight act layers.  The arithmetic tag is not included."""
    nt = lay.ntiles
    absw = {}
    tm = torch.zeros(TMAX_N, nt, dtype=torch.int32, device=ws.device)
    for name in OPERAND_REGIONS:
        layers, per = REGION_SHAPE[name]
        if name == "act":
            absw[ABSMAX["act"]] = max_bits(ws[lay.act: lay.act + lay.size["act"]])
            continue
        for l in range(layers):
            t = lay.tiles(ws, name, l)
            c = absmax_class(name, l)
            if c >= 0:
                absw[c] = max_bits(t)
            if name in TMAX:
                tm[TMAX[name] + l] = t.reshape(nt, per).abs().amax(dim=1).float().view(torch.int32)
    return absw, tm


def write_scale_words(lay, ws, tag=True):
    """write the absmax / tmax tables of the operand tiles in `ws` (and the SPLIT_F16 tag) into `ws`"""
    absw, tm = scale_words(lay, ws)
    wi = ws.view(torch.int32)
    wi[lay.absmax: lay.absmax + ABSMAX_FLOATS] = 0
    for c, bits in absw.items():
        wi[lay.absmax + c * ABSMAX_STRIDE] = bits
    if tag:
        wi[lay.absmax + ABSMAX["tag"] * ABSMAX_STRIDE] = ABSMAX_TAG_F16
    wi[lay.tmax: lay.tmax + lay.size["tmax"]] = 0
    wi[lay.tmax: lay.tmax + TMAX_N * lay.ntiles] = tm.reshape(-1)


# ---------------------------------------------------------------- the fold in fp64 (dw.hip fold_kernel / build_fold_table)
def param_tensors():
    """[(name, offset, shape)] of every tensor of the flat parameter vector, offsets from the library (dh_param_layout)"""
    from dynhor_amd import _lib
    out = []
    for net, pre, n in ((0, "sdf", N_SDF), (2, "col", N_COL)):
        for l in range(n):
            b, g, v, od, idim = _lib.param_layout(net, l)
            out += [(f"{pre}.lin{l}.bias", b, (od,)), (f"{pre}.lin{l}.weight_g", g, (od, 1)), (f"{pre}.lin{l}.weight_v", v, (od, idim))]
    return out


def variance_offset():
    from dynhor_amd import _lib
    return _lib.param_layout(1, 0)[2]


def assemble_dw(job_matrices, tpart_sums, dtype=torch.float64):
    """(dL/dW, dL/db) of the 14 linears (sdf lin0..8, colour lin0..4) from the 15 job matrices [256, nb*32] and the tile-partial
    slot sums [20, 256]."""
    M = [m.to(dtype) for m in job_matrices]
    T = tpart_sums.to(dtype)
    s = 1.0 / math.sqrt(2.0)
    out = []
    for l, (od, idim) in enumerate(SDF_DIMS):
        if l == 4:
            dW = torch.cat([M[4][:, :SKIP_OUT], M[8][:, :256 - SKIP_OUT]], 1) * s
            db = T[4]
        elif l == 8:
            dW = torch.cat([(T[9] + T[10])[None, :], M[9]], 0)
            db = torch.cat([T[11][:1], T[8]])
        else:
            dW = M[l][:od, :idim]
            db = T[l][:od]
        assert dW.shape == (od, idim) and db.shape == (od,), (l, dW.shape, db.shape)
        out.append((dW, db))
    for l, (od, idim) in enumerate(COL_DIMS):
        if l == 0:
            dW = torch.cat([M[11][:, :CAUX], M[10]], 1)
            db = T[12]
        elif l == 4:
            dW = T[16:19]
            db = T[19][:3]
        else:
            dW = M[11 + l]
            db = T[12 + l]
        assert dW.shape == (od, idim) and db.shape == (od,), (l, dW.shape, db.shape)
        out.append((dW, db))
    return out


def fold_reference(job_matrices, tpart_sums, params, dtype=torch.float64):
    """The flat gradient [n_params] in `dtype` (NaN in the variance slot, which the fold does not write): dL/dW and dL/db assembled
    from the job matrices and tile-partial sums, then (d g, d v) by autograd of sum(W * dL/dW) through W = g v / |v|."""
    lins = assemble_dw(job_matrices, tpart_sums, dtype)
    grad = torch.full((params.numel(),), float("nan"), dtype=dtype)
    layout = param_tensors()
    for k, (dW, db) in enumerate(lins):
        (_, boff, bshape), (_, goff, gshape), (_, voff, vshape) = layout[3 * k: 3 * k + 3]
        od, idim = vshape
        g = params[goff: goff + od].detach().to(dtype).cpu().reshape(od, 1).clone().requires_grad_(True)
        v = params[voff: voff + od * idim].detach().to(dtype).cpu().reshape(od, idim).clone().requires_grad_(True)
        W = g * v / v.norm(dim=1, keepdim=True)
        (W * dW.cpu()).sum().backward()
        grad[boff: boff + od] = db.cpu()
        grad[goff: goff + od] = g.grad.reshape(-1)
        grad[voff: voff + od * idim] = v.grad.reshape(-1)
    return grad
