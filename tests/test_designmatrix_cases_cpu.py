"""CPU: the references and cases of tests/designmatrix_cases.py are proved before anything trusts them — against the golden
outputs of the reference itself (tests/golden/designmatrix_ops.npz: lightkurve's DesignMatrix.standardize, patsy's bs()),
against scipy's savgol_coeffs where scipy is well conditioned, and every case against what its name says."""
import os

import numpy as np
import pytest
import scipy.signal as scipy_signal

import designmatrix_cases as C

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "designmatrix_ops.npz"))


def test_standardize_reference_reproduces_the_golden_matrix():
    """1e-12 is the project's figure for this golden file (tests/test_designmatrix_gpu.py); measured 8.9e-16."""
    S, want = G["S"], G["standardized"]
    ref = C.standardize_reference(S)
    assert np.max(np.abs(ref - want)) < 1e-12
    kinds = [C.column_kind(S[:, c]) for c in range(S.shape[1])]
    assert kinds[3] == "constant" and np.unique(S[:, 3]).tolist() == [2.5] and np.array_equal(ref[:, 3], want[:, 3])
    assert kinds[5] == "empty" and np.array_equal(ref[:, 5], want[:, 5]) and not ref[:, 5].any()
    assert all(k == "toleranced" for i, k in enumerate(kinds) if i not in (3, 5))


def test_numpy_nanstd_is_no_yardstick_for_constant_columns():
    """np.nanstd of 600 copies of 0.1 is not zero (a pairwise-summed mean that is an ulp off 0.1), of 5 copies it is: whether
    the reference leaves such a column unchanged hinges on numpy's summation order.  The documented contract — a column whose
    values are all equal is left unchanged — is what standardize_reference and the kernel keep."""
    assert np.nanstd(np.full((600, 3), 0.1), axis=0)[0] != 0.0
    assert np.array_equal(C.standardize_reference(np.full((600, 3), 0.1)), np.full((600, 3), 0.1))


def test_standardize_cases_are_what_their_names_say():
    cases = C.standardize_cases()
    assert {c.N for c, _, _ in cases} == set(C.STD_N) and {c.P for c, _, _ in cases} == set(C.STD_P)
    seen, parities = set(), {}
    for case, perm, ref in cases:
        A0, A1 = case.A
        assert case.A.shape == (2, case.N, case.P) and ref.shape == case.A.shape
        assert np.array_equal(A1, A0[:, perm], equal_nan=True) and sorted(perm) == list(range(case.P))
        assert np.array_equal(ref[1], ref[0][:, perm])                       # a column's reference does not depend on its place
        for c, fam in enumerate(case.families):
            v = A0[:, c]
            keep = ~np.isnan(v) & (v != 0)
            kind = C.column_kind(v)
            seen.add((fam, case.N, case.P))
            if case.N >= 3:
                assert kind == C.FAMILIES[fam][1], (case.name, fam)
            if kind == "constant":
                assert np.unique(v[keep]).size == 1
                assert np.array_equal(ref[0][:, c], np.where(np.isnan(v), 0.0, v))
            elif kind == "toleranced":
                med, mean, sd = C.column_stats(v)
                assert np.isfinite([med, mean, sd]).all() and sd > 0 and abs(mean) / sd <= 1e6, (case.name, fam)
                assert not ref[0][~keep, c].any() and np.isfinite(ref[0][:, c]).all()
                parities.setdefault(fam, set()).add(int(keep.sum()) % 2)
            else:
                assert not ref[0][:, c].any()                                # empty / nonfinite: zeros
            if case.N >= 3:
                if fam in ("normal_odd", "normal_even", "nan_odd", "nan_even"):
                    assert int(keep.sum()) % 2 == (1 if fam.endswith("odd") else 0) and (v == 0).sum() >= case.N // 20
                    assert np.isnan(v).any() == fam.startswith("nan")
                if fam == "one_kept":
                    assert keep.sum() == 1
                if fam == "two_equal_kept":
                    assert keep.sum() == 2
                if fam.startswith("const_") and fam.endswith("_zeros"):
                    assert (v == 0).sum() == case.N // 2 and keep.sum() == case.N - case.N // 2
                if fam.startswith("const_") and fam.endswith("_nan"):
                    assert np.isnan(v).sum() == case.N // 3 and keep.sum() == case.N - case.N // 3
                if fam.startswith("const_"):
                    assert float(np.unique(v[keep])[0]) == float(fam.split("_")[1])
                if fam == "offset_1e6":
                    assert abs(np.mean(v) - 1e6) < 1e-6 and 1.0 < np.std(v) < 1.1
                if fam == "neg_zero":
                    assert np.signbit(v[v == 0]).all() and (v == 0).sum() == (case.N + 3) // 4 and not ref[0][v == 0, c].any()
                if fam == "pos_inf":
                    assert np.isposinf(v).sum() == 1 and not np.isneginf(v).any()
                if fam == "both_inf":
                    assert np.isposinf(v).sum() == 1 and np.isneginf(v).sum() == 1
    for N in C.STD_N:
        if N >= 3:
            for fam in C.FAMILIES:                     # every family at every N, alone and among 13 columns
                assert (fam, N, 1) in seen and (fam, N, 13) in seen, (fam, N)
    assert parities["normal_odd"] == {1} and parities["normal_even"] == {0}


def _golden_knots(x, n_knots, degree, include_intercept=True):
    """create_spline_matrix's knots without `knots=`: equally spaced percentiles of x between its extremes."""
    n_inner = n_knots - degree - 1 + (0 if include_intercept else 1)
    return np.r_[x.min(), np.percentile(x, np.linspace(0, 100, n_inner + 2)[1:-1]), x.max()]


def test_bspline_reference_reproduces_patsy():
    """1e-12 is the project's figure for these golden matrices; measured 3.0e-15, 3.3e-16, 3.3e-16."""
    x = G["x"]
    assert np.max(np.abs(C.bspline_reference(x, _golden_knots(x, 20, 3), 3) - G["spline_n20_d3"])) < 1e-12
    assert np.max(np.abs(C.bspline_reference(x, _golden_knots(x, 12, 5, False), 5)[:, 1:] - G["spline_n12_d5_noint"])) < 1e-12
    given = np.r_[x.min(), np.sort(G["knots_given"]), x.max()]
    assert np.max(np.abs(C.bspline_reference(x, given, 3) - G["spline_knots_d3"])) < 1e-12


def test_spline_cases_are_what_their_names_say():
    cases = {c.name: c for c in C.spline_cases()}
    assert len(cases) == len(C.spline_cases())
    assert {c.degree for c in cases.values()} == set(range(8))
    assert {c.knots.shape[1] - 2 for c in cases.values()} >= {0, 1, 6, 20}
    assert {c.x.size for c in cases.values()} == set(C.SPL_N)
    assert any(c.knots.shape[0] == 3 and len({k.tobytes() for k in c.knots}) == 3 for c in cases.values())
    for c in cases.values():
        assert np.all(np.diff(c.knots, axis=1) >= 0)                                   # knot vectors are monotone
        lo, hi = c.knots[0, 0], c.knots[0, -1]
        assert np.all(c.knots[:, 0] == lo) and np.all(c.knots[:, -1] == hi)
        assert np.isfinite(c.x).all() and c.x.min() >= lo and c.x.max() <= hi
        if c.x.size > 1:
            assert np.any(np.diff(c.x) < 0) and lo in c.x and hi in c.x               # unsorted, both ends present
        if c.x.size >= 255:
            for k in np.unique(c.knots[0, 1:-1]):
                assert k in c.x
                assert k == lo or np.nextafter(k, -np.inf) in c.x
                assert k == hi or np.nextafter(k, np.inf) in c.x
    for d in range(8):
        mult = lambda name: np.unique(cases["%s_d%d" % (name, d)].knots[0, 1:-1], return_counts=True)
        assert 2 in mult("double")[1]
        assert d + 1 in mult("full_multiplicity")[1]
        assert cases["equals_lo_d%d" % d].knots[0, 1] == cases["equals_lo_d%d" % d].knots[0, 0]
        assert cases["equals_hi_d%d" % d].knots[0, -2] == cases["equals_hi_d%d" % d].knots[0, -1]
        inner = cases["ulp_apart_d%d" % d].knots[0, 1:-1]
        assert np.any(np.nextafter(inner[:-1], np.inf) == inner[1:])
    assert cases["d3_k6_N1"].x[0] in cases["d3_k6_N1"].knots[0, 1:-1]                   # the single sample sits on a knot


@pytest.mark.parametrize("name", [c.name for c in C.spline_cases()])
def test_bspline_reference_is_a_partition_of_unity_on_its_span(name):
    """Properties no rounding of the exact values can break by more than an ulp per entry: non-negative, zero outside the
    degree + 1 columns of the sample's span, rows summing to 1 (degree + 1 roundings: 8 x 2**-53 at the most)."""
    case = next(c for c in C.spline_cases() if c.name == name)
    ref = C.spline_reference_of(name)
    for b, knots in enumerate(case.knots):
        T = C.full_knots(knots, case.degree)
        assert ref[b].shape == (case.x.size, knots.size - 2 + case.degree + 1)
        assert np.all(ref[b] >= 0) and np.max(np.abs(ref[b].sum(axis=1) - 1.0)) <= 8 * 2.0 ** -53
        for n, xv in enumerate(case.x):
            mu = C.bspline_span(xv, T, case.degree)
            assert T[mu] < T[mu + 1] and (T[mu] <= xv < T[mu + 1] or xv == T[-1] == T[mu + 1])
            assert not ref[b, n, :mu - case.degree].any() and not ref[b, n, mu + 1:].any()


def test_savgol_reference_agrees_with_scipy_at_polyorder_2():
    """scipy.signal.savgol_coeffs solves a Vandermonde least-squares problem in double; at polyorder 2 its conditioning leaves
    3.4e-16 (window 5), 2.7e-15 (11) and 1.1e-13 (101) of the largest tap (measured): the bounds are those, rounded up."""
    for window, tol in ((5, 1e-15), (11, 1e-14), (101, 5e-13)):
        taps, _ = C.savgol_reference(window, 2, rows=())
        err = np.max(np.abs(taps - scipy_signal.savgol_coeffs(window, 2))) / np.max(np.abs(taps))
        print("savgol reference vs scipy (%d, 2): %.2g" % (window, err))
        assert err <= tol


def test_savgol_reference_edge_rows_are_the_polynomial_refit():
    """edge[0][r] @ y is np.polyfit's value at position r over the first w samples, edge[1][r] at position w - half + r over the
    last w (scipy's mode='interp'), at a low order where polyfit in double is accurate (1e-12 of |y| <= 1)."""
    rng = np.random.default_rng(4)
    for window, polyorder in ((5, 2), (11, 3), (31, 2)):
        half = window // 2
        _, edge = C.savgol_reference(window, polyorder)
        y = rng.uniform(-1, 1, window)
        fit = np.polyval(np.polyfit(np.arange(window), y, polyorder), np.arange(window))
        assert np.max(np.abs(edge[0] @ y - fit[:half])) < 1e-12 and np.max(np.abs(edge[1] @ y - fit[window - half:])) < 1e-12
        z = rng.uniform(-1, 1, 3 * window)
        out = C.savgol_apply(z, *C.savgol_reference(window, polyorder))
        assert np.max(np.abs(out - scipy_signal.savgol_filter(z, window, polyorder, mode="interp"))) < 1e-12


def test_savgol_cases_cover_the_accepted_range():
    cases = C.savgol_cases()
    assert len(set(c[:2] for c in cases)) == len(cases) == 70
    for w in (3, 5, 17, 31, 101):
        assert [c[1] for c in cases if c[0] == w] == list(range(min(15, w - 1) + 1))
        assert all(c[2] == tuple(range(w // 2)) for c in cases if c[0] == w)
    for w in (401, 2449):
        assert [c[1] for c in cases if c[0] == w] == list(range(7))
        assert all(c[2] == (0, 1, w // 2 - 1) for c in cases if c[0] == w)
