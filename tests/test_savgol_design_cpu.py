"""CPU: lk_savgol_design (the host-side design of the FIR taps and edge operators every flatten kernel applies; no GPU needed
once the library is built) against the exact rational solution of tests/designmatrix_cases.py, for every polyorder the
launcher accepts.

Bound (stated): |got - exact| <= 2**-52 * max|row| for the taps and for every checked edge row.  A per-tap error of eps times the
largest weight perturbs sum c_j y_j by no more than the fp64 summation of the filter itself does, so a design inside the bound is
as good as the exact one rounded once.

Measured, as max |got - exact| / max|row| in units of 2**-52 over the taps and checked rows:
  * the Gram-polynomial design: at most 0.75 over all 70 cases (a value that rounds twice, long double then double, can be one
    ulp off, and one ulp of an entry just above a power of two is up to 2**-52 of it).
  * the monomial normal equations in long double that it replaced failed 25 of the 70 cases: <= 0.98 up to polyorder 6 except
    6.3 at (2449, 6), then (101, 7) 2.2, (31, 8) 1.9, (101, 8) 6.7, (31, 9) 32, (17, 10) 5.4, (31, 10) 240, (101, 10) 134,
    (17, 12) 1.7e3, (31, 12) 7.9e3, (101, 12) 1.2e3, (17, 15) 1.2e7, (31, 15) 1.2e6, (101, 15) 9.1e5: seven digits lost at
    polyorder 15.  They also took 4 s per design at window 2449 (one solve per edge row); the recurrence takes 0.1 s."""
import numpy as np
import pytest

import designmatrix_cases as C
from lightkurve_amd import _capi

BOUND = 2.0 ** -52


@pytest.mark.parametrize("window,polyorder,rows", C.savgol_cases(), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_design_is_the_exact_solution_rounded_once(window, polyorder, rows):
    taps, edge = C.savgol_reference_of(window, polyorder)
    got_taps, got_edge = _capi.savgol_design(window, polyorder)
    assert got_taps.shape == taps.shape and got_edge.shape == edge.shape
    worst = np.max(np.abs(got_taps - taps)) / np.max(np.abs(taps))
    for side in range(2):
        for r in rows:
            worst = max(worst, np.max(np.abs(got_edge[side, r] - edge[side, r])) / np.max(np.abs(edge[side, r])))
    print("savgol design (%d, %d): max |got - exact| / max|row| = %.3g x 2**-52" % (window, polyorder, worst / BOUND))
    assert worst <= BOUND


def test_taps_and_edge_rows_fit_polynomials_exactly():
    """What the design is for, independent of the rational reference: a polynomial of degree <= polyorder sampled on the window
    is reproduced — the taps return its value at the centre, edge row r its value at position r.  Bound: H is a projector, so
    a row's 2-norm is <= 1 and its 1-norm <= sqrt(w); with |y| <= 1 the fp64 dot product errs by <= w 2**-53 sqrt(w) and the
    design's own error (2**-52 of the largest weight, <= 1, per tap) adds <= w 2**-52."""
    for window, polyorder in ((17, 15), (31, 9), (101, 12)):
        taps, edge = _capi.savgol_design(window, polyorder)
        half = window // 2
        u = (np.arange(window) - half) / half
        bound = window * (np.sqrt(window) / 2 + 1) * BOUND
        for deg in range(polyorder + 1):
            y = np.polynomial.chebyshev.Chebyshev.basis(deg)(u)           # |y| <= 1: the errors below are absolute
            assert abs(taps[::-1] @ y - y[half]) <= bound, (window, polyorder, deg)
            assert np.max(np.abs(edge[0] @ y - y[:half])) <= bound, (window, polyorder, deg)
            assert np.max(np.abs(edge[1] @ y - y[window - half:])) <= bound, (window, polyorder, deg)


def test_rejected_arguments():
    for window, polyorder in ((4, 2), (5, 5), (33, 16), (0, 0)):
        with pytest.raises((ValueError, RuntimeError)):
            _capi.savgol_design(window, polyorder)
