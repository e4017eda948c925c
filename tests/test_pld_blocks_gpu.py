"""GPU: every PCA block that lk_pld_design_batch writes, against numpy, on each side of every boundary between the kernel
routes of pld.hip (tests/pld_block_cases.py has the shapes, the inputs and the restatement; tests/test_pld_blocks_cpu.py checks
the preconditions without a GPU).  The end-to-end tests of tests/test_pld_gpu.py see these kernels only through the corrected
flux, to 1e-6 of the median; here each block Q (N x ko) is held against its own source matrix S (N x Pc, G = S S^T, singular
values s), for B = 2 cutouts per call:

  1. max |Q^T Q - I| < 1e-10;
  2. Q lies in the column space of S: ||Q - U_r U_r^T Q||_F <= 1e-9 sqrt(ko) (a wrong mean projection or projection tile leaves it);
  3. ||G Q - Q (Q^T G Q)||_F <= bar s[0]^2 sqrt(ko) — subspace iteration (Pc > 138): 1e-6 at the default stop criterion, 1e-8
     under pld_set_eig_tolerance(1e-10); direct solvers: the bar derived from the Gram formation (pld_block_cases.backward_bar);
  4. trace(Q^T G Q) >= (1 - 1e-5) sum s[:ko]^2;
  5. ||P_svd - P_Q||_2 <= 1e-6 wherever s has a gap of more than 5 % at the cut;
and the design width, the prior block and the constant column.

Measured on an MI355X, worst block per route over all cases, assertion 3 as a fraction of s[0]^2 sqrt(ko):
  product blocks   plain products + Jacobi (1 column)         8.1e-16   derived bar >= 6.6e-13
                   plain products + direct solver             4.0e-15   0.2 % of its derived bar at worst
                   moment form + direct solver                1.2e-14   0.9 % of its derived bar (>= 3.7e-13) at worst
                   moment form + subspace iteration           8.9e-08 at the default criterion (bar 1e-6; the 4060-column block),
                                                              6.9e-11 at 1e-10 (bar 1e-8)
  pixel blocks     float32-source Gram + direct solver        2.0e-15   (bar 1e-9 .. 1e-8)
                   pld_ratio_kernel + direct solver (P = 3)   2.8e-15
                   float32-source Gram + iteration (P = 144)  2.1e-13 at either criterion
                   pld_ratio_kernel + iteration (P = 145/148) 7.9e-14 at either criterion
No block needed a bar wider than the derived one.  The other figures: |Q^T Q - I| <= 4.8e-14, range <= 2.3e-15, lost variance
<= 1.6e-13, subspace distance <= 1.4e-11 (pixel blocks) and <= 2.5e-14 (the 36 of 126 product blocks with a gap, all on the
direct solvers)."""
import numpy as np
import pytest

import pld_block_cases as C

pytestmark = pytest.mark.gpu

def _design(case, data, tol=0.0):
    from lightkurve_amd import _capi
    h = _capi.Handle.get(0)
    h.pld_set_eig_tolerance(tol)
    try:
        return _capi.pld_design_batch(data["pix"], data["bkg"], data["flux"], data["time"], data["knots"], case.order, case.c,
                                      C.DEGREE, case.normalize)
    finally:
        h.pld_set_eig_tolerance(0.0)


def _check_case(case):
    from lightkurve_amd import _capi
    data = C.batch(case)
    K = _capi.pld_design_width(case.P, case.Pb, case.order, case.c, C.N_INNER + C.DEGREE + 1)
    assert K == C.design_width(case)
    iterated = any(C.route(case, blk)["solver"] == "subspace" for blk in C.blocks(case))
    for tol in ((0.0, 1e-10) if iterated else (0.0,)):
        X, ps = _design(case, data, tol)
        assert X.shape == (2, case.N, K) and ps.shape == (2, K)
        assert np.all(np.isfinite(X)) and np.all(X[:, :, -1] == 1.0)
        for b in range(2):
            cut = {k: v[b] for k, v in data.items()}
            ref = C.prior_reference(case, cut["flux"])
            ulp = float(np.spacing(np.float32(ref[-1] / 10.0))) * 10.0       # of the float32 standard deviation, times 10
            assert np.max(np.abs(ps[b] - ref) / np.where(np.arange(K) < C.blocks(case)[-1].col0, 1.0 / case.c, 1.0)) <= 2.0 * ulp
            for blk, S, unc in C.sources(case, cut, X[b]):
                C.check_block(case, blk, X[b][:, blk.col0:blk.col0 + blk.ko], S, unc, tol=tol, label="%s[%d]" % (case.name, b))
    

@pytest.mark.parametrize("case", C.ROUTE_CASES, ids=lambda c: c.name)
def test_blocks_on_both_sides_of_every_route_boundary(case):
    """Plain products below kMomentMinCols and the moment form above, orders 2 to 4, both PRE, both expansions, with and
    without the float32 copy of C, KT 1 to 3, WR 1, 2 and 4, the three eigen-solvers, the widest block admitted."""
    _check_case(case)


@pytest.mark.parametrize("case", C.PIXEL_CASES, ids=lambda c: c.name)
def test_pixel_blocks_on_every_gram_and_projection_route(case):
    """First-order and background block on the same integer-valued pixels: the float32-source route (4 <= P <= 144) and
    pld_ratio_kernel + pld_project_kernel on either side of it, VEC4 true and false, background divided by its row sums
    (pld_rowdiv_kernel) and not."""
    _check_case(case)


@pytest.mark.parametrize("case", C.TAIL_CASES, ids=lambda c: c.name)
def test_cadence_tails_of_the_staged_kernels(case):
    """N around the 64-cadence LDS stage of the moment Gram and around the 64 WR rows of a projection workgroup, WR = 2, 4, 1."""
    _check_case(case)


def test_block_too_wide_is_refused():
    """29 components at order 3: 4495 product columns, beyond the 4096 the kernels are sized for."""
    from lightkurve_amd import _capi
    case = C.REFUSED
    data = C.batch(case)
    with pytest.raises(ValueError, match="4495 columns"):
        _capi.pld_design_batch(data["pix"], data["bkg"], data["flux"], data["time"], data["knots"], case.order, case.c, C.DEGREE,
                               case.normalize)


def test_cutouts_of_a_batch_do_not_see_each_other():
    """The design matrix of cutout 1 in a call of two equals, bit for bit, that of the same cutout alone."""
    case = C.INDEPENDENCE
    data = C.batch(case)
    X2, ps2 = _design(case, data)
    X1, ps1 = _design(case, {k: v[1:2] for k, v in data.items()})
    assert np.array_equal(X2[1], X1[0]) and np.array_equal(ps2[1], ps1[0])
    assert not np.array_equal(X2[0], X2[1])
