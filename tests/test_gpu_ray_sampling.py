"""GPU: the sampling kernels of csrc/kernels_ray.hip one by one -- dh_merge_samples, dh_coarse_samples, dh_midpoints,
dh_upsample_step -- against oracle/neus_oracle.py in fp64, at odd sizes, ties, NULL paths and degenerate CDFs.  Every output buffer
sits between canary pads (tests/ray_kernels_util.py); no sample is left out of any assertion; the inputs, margins and criteria are
licensed on the CPU by tests/test_cpu_ray_kernels_ref.py."""
import pytest
import torch

from tests import ray_kernels_util as U

pytestmark = pytest.mark.gpu

F32, F64 = U.F32, U.F64


def _cuda(*ts):
    return tuple(None if t is None else t.cuda().contiguous() for t in ts)


# ------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("n_cur", U.MERGE_N_CUR)
def test_merge_is_the_stable_sort_bit_for_bit(n_cur):
    """A pure permutation: torch.equal against torch.sort(cat[z, z_new], stable=True) and the gathered sdf, for new depths bitwise
    equal to old ones, duplicates inside each list, all new depths before / after all old ones, and with sdf_out NULL."""
    ties = 0
    for k in U.MERGE_N_NEW:
        for B in U.MERGE_B:
            for mode in U.MERGE_MODES:
                z, zn, s, sn = _cuda(*U.merge_inputs(B, n_cur, k, mode))
                assert bool((zn[:, 1:] >= zn[:, :-1]).all()) and bool((z[:, 1:] >= z[:, :-1]).all()), "the kernel's contract: both lists ascending"
                want_z, want_s = U.merge_reference(z, zn, s, sn)
                got_z, got_s = U.hip_merge(z, zn, s, sn, with_sdf=True)
                assert torch.equal(got_z, want_z), (n_cur, k, B, mode, "depths")
                assert U.merge_matches(got_z, got_s, want_z, want_s), (n_cur, k, B, mode, "gathered sdf")
                got_z2, none = U.hip_merge(z, zn, s, sn, with_sdf=False)
                assert none is None and U.merge_matches(got_z2, None, want_z, want_s), (n_cur, k, B, mode, "sdf_out NULL")
                if mode == "ties":
                    ties += int((z[:, :, None] == zn[:, None, :]).sum())
    assert ties > 0 or n_cur == 1, "the tie cases must contain new depths bitwise equal to old ones"


# ------------------------------------------------------------------------------------------------ coarse samples, mid-points
# z = near + (far - near) * (j / (n - 1)) + (t - 0.5) * 2 / n.  Roundings of fp32: the quotient j / (n - 1), far - near, their
# product, the first sum, t - 0.5 (times 2 is exact), the quotient by n, the last sum: 7, each at most half an ulp of a value
# below 4 (asserted on the reference), i.e. 2^-23.  A fused multiply-add only removes roundings.  Bound: 7 x 2^-23 = 8.3e-7.
# pts = o + d z from the kernel's own z: product and sum, 2 x 2^-23 (|d_c| <= 1, |o_c| < 4).
COARSE_Z_BOUND = 7 * 2.0 ** -23
POINT_BOUND = 2 * 2.0 ** -23
# mid = z_j + 0.5 (z_{j+1} - z_j): the difference and the sum (the half is exact): 2 roundings of mid, each reaching a point
# scaled by |d_c| <= 1; then product and sum of o + d mid: 4 x 2^-23 = 4.8e-7 in all.
MIDPOINT_BOUND = 4 * 2.0 ** -23


@pytest.mark.parametrize("n", (1, 2, 3, 64, 127))
def test_coarse_samples_against_fp64(n):
    for B in (1, 3, 5, 257):                                  # B n = 1, 3, 5, ... : mostly not multiples of the 256-thread block
        o, d, near, far, t = _cuda(*U.coarse_inputs(B))
        for t_rand in (t, None):
            z, pts = U.hip_coarse(o, d, near, far, t_rand, n)
            ref = U.coarse_reference(o, d, near, far, t_rand, n)
            assert ref.abs().max().item() < 4.0 and o.abs().max().item() < 4.0 and d.abs().max().item() <= 1.0
            err = (z.double() - ref).abs().max().item()
            own = (pts.double().view(B, n, 3) - (o.double()[:, None] + d.double()[:, None] * z.double()[..., None])).abs().max().item()
            print(f"coarse n {n} B {B} t_rand {'set' if t_rand is not None else 'NULL'}: max |z - z64| {err:.2e} (bound {COARSE_Z_BOUND:.2e}); "
                  f"max |pts - (o + d z)| {own:.2e} (bound {POINT_BOUND:.2e})")
            assert err <= COARSE_Z_BOUND and own <= POINT_BOUND
    assert (257 * n) % 256 != 0


@pytest.mark.parametrize("n", (1, 2, 3, 64, 127, 128))
def test_midpoints_against_fp64(n):
    for B in (1, 3, 5, 257):
        o, d, near, far, t = U.coarse_inputs(B, seed=n)
        z = U.coarse_reference(o, d, near, far, t if n >= 64 else None, n).to(F32)    # (small n: the perturbation alone reaches +-1, depths would pass 4)
        if n >= 3:
            z[:, 1] = z[:, 2]                                  # a section of length zero
        o, d, z = _cuda(o, d, z)
        for sample_dist in (2.0 / 64, 0.1):
            sd = float(torch.tensor(sample_dist, dtype=F32))
            pts = U.hip_midpoints(o, d, z, sd)
            ref = U.midpoints_reference(o, d, z, sd)
            assert ref.abs().max().item() < 4.0 and z.abs().max().item() + sd < 4.0
            err = (pts.double() - ref).abs().max().item()
            last = (pts.double() - ref).view(B, n, 3)[:, -1].abs().max().item()
            print(f"mid-points n {n} B {B} sample_dist {sd:.4f}: max err {err:.2e}, last section {last:.2e} (bound {MIDPOINT_BOUND:.2e})")
            assert err <= MIDPOINT_BOUND
        if B == 257:
            assert (B * n) % 256 != 0 or n == 128


# ------------------------------------------------------------------------------------------------ up-sampling
def _kernel(o, d, z, sdf, k, inv_s):
    return U.hip_upsample(o, d, z, sdf, k, inv_s)


@pytest.mark.parametrize("n_cur", U.UPS_N_CUR)
def test_upsample_step_against_fp64_in_cdf_space(n_cur):
    """The kernel and the fp64 oracle get identical fp32 (z, sdf): bumpy sphere, thin slab (many empty sections), rays that miss,
    a ray opaque in its first section -- every family in every case, no family left out at any n_new or inv_s.  The criteria (range,
    order, CDF space with tol = 4 x the fp32 oracle's residual and tol < 0.25 / n_new, z space, points) are in
    ray_kernels_util.check_upsample_case and hold for EVERY sample."""
    cases = [c for c in U.upsample_cases() if c[1] == n_cur]
    assert len(cases) == 16 + 3
    worst = None
    for case in cases:
        m = U.check_upsample_case(case, _kernel, device="cuda")
        r = m["res"] / m["tol"]
        if worst is None or r > worst[0]:
            worst = (r, m)
        if case[0] != 257 or case[3] == 512.0:
            print(f"  B {case[0]:3d} n_cur {n_cur:3d} n_new {case[2]:2d} inv_s {case[3]:5.0f} x{len(case[4]):2d}: CDF residual {m['res']:.2e} <= tol {m['tol']:.2e} "
                  f"(cap {m['cap']:.2e}); max |dz| {m['dz']:.2e} (fp32 oracle {m['dz32']:.2e}); share > 1e-4 {m['share']:.2e} ({m['share32']:.2e})")
    print(f"n_cur {n_cur}: worst residual / tol {worst[0]:.3f} at {worst[1]['case'][:4]}")
