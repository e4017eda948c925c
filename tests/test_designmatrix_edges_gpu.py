"""GPU: lk_standardize_batch (dm_standardize_kernel) and lk_spline_basis_batch (bspline_row through pld_spline_kernel) against
the plain references of tests/designmatrix_cases.py (proved on the CPU by tests/test_designmatrix_cases_cpu.py) at the tile
edges of the kernels and at the values where their rules decide: constant columns of values that are not representable, NaN,
-0.0 and +-inf for standardize; samples on, and one ulp either side of, single, repeated and nearly coincident knots for the
spline basis.  Tolerances are the ones tests/test_designmatrix_gpu.py states for the golden file (1e-12), everything the
documented contract fixes is compared with `==`."""
import numpy as np
import pytest

import designmatrix_cases as C
from lightkurve_amd import _capi
from lightkurve_amd.correctors.designmatrix import create_spline_matrix

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.mark.parametrize("N", C.STD_N)
def test_standardize_against_the_plain_reference(N):
    """Every column family alone (P = 1) and among 13 columns, B = 2 with the second matrix a column permutation of the first.
    `==`: missing entries, unchanged constant columns (0.1, 3.3 and 1e-3 included: a kernel that decides "constant" by
    sd == 0 returns zeros for them wherever the rounded mean is an ulp off the value, which depends on N and on the
    reduction tree; min == max does not), all-zero and all-NaN columns, columns holding +-inf (zeros, where (v - med) / sd
    would be NaN), and the permuted copy bit for bit.  Everything else within 1e-12 max(1, |mean| / sd) of the reference: 1e-12 is the golden
    test's figure, the factor is the conditioning of v - mean.  Measured maximum of |got - ref| / max(1, |mean| / sd) over all
    N: 8.9e-16."""
    worst = 0.0
    for case, perm, ref in C.standardize_cases():
        if case.N != N:
            continue
        got = _capi.standardize_batch(case.A)
        assert got.shape == ref.shape
        assert np.array_equal(got[1], got[0][:, perm]), case.name                  # same bits wherever the column stands
        for c, fam in enumerate(case.families):
            v, g, r = case.A[0][:, c], got[0][:, c], ref[0][:, c]
            if C.column_kind(v) != "toleranced":
                assert np.array_equal(g, r), (case.name, fam, C.column_kind(v))
                continue
            keep = ~np.isnan(v) & (v != 0)
            assert np.all(g[~keep] == 0), (case.name, fam)
            _, mean, sd = C.column_stats(v)
            err = np.max(np.abs(g - r)) / max(1.0, abs(mean) / sd)
            worst = max(worst, err)
            assert err <= TOL, (case.name, fam, err)
    print("standardize N = %d: max |got - ref| / max(1, |mean| / sd) = %.3g" % (N, worst))


@pytest.mark.parametrize("name", [c.name for c in C.spline_cases()])
def test_spline_basis_against_cox_de_boor_in_rational_arithmetic(name):
    """Degrees 0..7, 0 / 1 / 6 / 20 interior knots, N on both sides of the 256-row tile, unsorted x holding both bounds, every
    interior knot and its two neighbours in double; double knots, knots of multiplicity degree + 1, an interior knot on either
    bound, two knots one ulp apart, three knot vectors in one call.  Within 1e-12 of the exact basis (the golden test's figure),
    exactly zero outside the degree + 1 columns of the sample's span, non-negative, rows summing to 1 within the same 1e-12.
    Measured maximum over all cases: |got - ref| 4.4e-16, |row sum - 1| 8.9e-16."""
    case = next(c for c in C.spline_cases() if c.name == name)
    ref = C.spline_reference_of(name)
    B = case.knots.shape[0]
    got = _capi.spline_basis_batch(np.tile(case.x, (B, 1)), case.knots, degree=case.degree)
    assert got.shape == ref.shape
    for b in range(B):
        T = C.full_knots(case.knots[b], case.degree)
        for n, xv in enumerate(case.x):
            mu = C.bspline_span(xv, T, case.degree)
            assert np.all(got[b, n, :mu - case.degree] == 0) and np.all(got[b, n, mu + 1:] == 0), (b, n, xv)
    err, rows = np.max(np.abs(got - ref)), np.max(np.abs(got.sum(axis=2) - 1.0))
    print("spline %s: max |got - ref| = %.3g, max |row sum - 1| = %.3g" % (name, err, rows))
    assert np.all(got >= 0)
    assert err <= TOL and rows <= TOL


def test_create_spline_matrix_rejects_knots_outside_the_data():
    """patsy's bs() raises for an interior knot outside [min(x), max(x)] and accepts one equal to a bound; the front end used to
    pass a non-monotone knot vector to the kernel."""
    x = np.linspace(2.0, 5.0, 40)[::-1].copy()
    for bad in ([1.9, 3.0], [3.0, 5.1], [np.nextafter(2.0, -np.inf)], [np.nextafter(5.0, np.inf)]):
        with pytest.raises(ValueError):
            create_spline_matrix(x, knots=bad, degree=3)
    for knots in ([2.0, 3.0], [3.0, 5.0], [2.0, 5.0]):
        dm = create_spline_matrix(x, knots=knots, degree=3)
        ref = C.bspline_reference(x, np.r_[2.0, knots, 5.0], 3)
        assert dm.shape == ref.shape and np.max(np.abs(dm.values - ref)) <= TOL
