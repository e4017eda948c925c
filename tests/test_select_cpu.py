"""CPU: the numpy restatements of tests/select_cases.py (what test_select_gpu.py holds the kernels to) — against astropy's
``sigma_clip`` where astropy is importable, their own edge cases, the test inputs' condition, and the host-side argument
checks of the new entry points (no device call)."""
import numpy as np
import pytest

import select_cases as C
from oracle import np_oracle as O


def test_asymmetric_restatement_equals_astropy():
    stats = pytest.importorskip("astropy.stats")
    rng = np.random.default_rng(3)
    for n in (40, 1025, 4500):
        y = C._noisy(rng, n)
        y[rng.choice(n, 3, replace=False)] = np.nan
        for p in C.PARAMS:
            want = stats.sigma_clip(y, cenfunc="median", stdfunc="std", masked=True,
                                    **dict(dict(sigma=3.0, maxiters=5), **p)).mask
            assert np.array_equal(C.sigma_clip_mask_asym(y, **p), want), (n, p)


def test_symmetric_case_equals_the_oracle():
    b = C.ragged_batch()
    for s in C.row_slices(b["n_off"]):
        if s.stop == s.start:
            continue
        for sigma, maxiters in ((5.0, 5), (3.0, 5), (4.0, 1)):
            with np.errstate(all="ignore"):
                want = O.sigma_clip_mask(b["flux"][s], sigma=sigma, maxiters=maxiters)
            assert np.array_equal(C.sigma_clip_mask_asym(b["flux"][s], sigma=sigma, maxiters=maxiters), want)


def test_restatement_edge_cases():
    f = C.sigma_clip_mask_asym
    assert f(np.zeros(0)).shape == (0,)
    assert f(np.full(7, np.nan)).all()                                      # nothing finite: everything flagged
    assert not f(np.full(9, 1.0003)).any()                                  # std 0: equality keeps
    assert np.array_equal(f(np.array([1.0, np.inf, 1.0, -np.inf, np.nan])), [False, True, False, True, True])
    y = np.r_[np.zeros(50), 10.0, -10.0]
    assert np.array_equal(np.flatnonzero(f(y, sigma=3.0)), [50, 51])
    assert np.array_equal(np.flatnonzero(f(y, sigma_lower=100.0, sigma_upper=3.0)), [50])      # only the up-going one
    assert np.array_equal(np.flatnonzero(f(y, sigma_lower=3.0, sigma_upper=100.0)), [51])
    assert not f(y, maxiters=0).any()                                       # no round: only non-finite values
    # maxiters caps the rounds; None runs to the fixed point
    rng = np.random.default_rng(11)
    z = np.r_[rng.standard_normal(2000), 6.0 + 0.5 * np.arange(40)]
    n1, n5, nn = (int(f(z, sigma=3.0, maxiters=m).sum()) for m in (1, 5, None))
    assert n1 < n5 <= nn
    rounds = []
    f(z, sigma=3.0, maxiters=2, rounds=rounds)
    assert len(rounds) == 2


def test_inputs_stay_clear_of_the_bounds_and_clip_about_one_percent():
    b = C.ragged_batch()
    assert b["rows"].count("all-nan") == 1 and b["rows"].count("constant") == 1 and "noise+inf" in b["rows"]
    counts = np.diff(b["n_off"])
    assert sorted(set(counts) & set(C.LENGTHS)) == sorted(C.LENGTHS) and counts[-1] == 0 and 0 in counts[1:-1]
    for p in C.PARAMS:
        for s in C.row_slices(b["n_off"]):
            assert C.clear_of_bounds(b["flux"][s], **p)
    sym = C.restated_mask(b["flux"], b["n_off"], **C.PARAMS[0])
    asym = C.restated_mask(b["flux"], b["n_off"], **C.PARAMS[1])
    big = C.row_slices(b["n_off"])[11]                                      # 4500 cadences
    fin = np.isfinite(b["flux"][big])
    assert 0.005 < (sym[big] & fin).mean() < 0.02
    assert (asym[big] & fin).sum() < (sym[big] & fin).sum()                 # the down-going outliers survive 20 sigma


def test_cdpp_tail_restatement():
    from lightkurve_amd.lightcurve import running_mean
    rng = np.random.default_rng(4)
    y = 1.0 + 3e-4 * rng.standard_normal(500)
    assert np.array_equal(C.running_mean(y, 13), running_mean(y, 13))
    assert np.isnan(C.cdpp_tail(np.zeros(0), None, 13))
    assert np.isnan(C.cdpp_tail(y, np.ones(500, dtype=bool), 13))
    assert C.cdpp_tail(y, None, 500) == 0.0 and C.cdpp_tail(y, None, 900) == 0.0      # w = n_kept: one mean
    assert C.cdpp_tail(np.full(40, 1.0003), None, 13) == 0.0
    ppm = y / np.median(y) * 1e6
    assert C.cdpp_tail(y, None, 1) == pytest.approx(np.std(ppm), rel=1e-10)
    assert 60 < C.cdpp_tail(y, None, 13) < 110                              # 300 ppm / sqrt(13)
    # float64 against long double on the GPU test's own inputs: the reference's rounding leaves room under rtol 1e-9
    b = C.ragged_batch()
    outl = C.restated_mask(b["flux"], b["n_off"], **C.PARAMS[0])
    worst = 0.0
    for td in C.DURATIONS:
        for s in C.row_slices(b["n_off"]):
            kept = b["flux"][s][~outl[s]].astype(np.longdouble)
            if kept.size <= td:
                continue
            cs = np.cumsum(np.insert(kept / np.median(kept) * np.longdouble(1e6), 0, 0))
            ref = float(np.std((cs[td:] - cs[:-td]) / np.longdouble(td)))
            if ref == 0.0:                                                  # the constant row: both are exactly 0
                assert C.cdpp_tail(b["flux"][s], outl[s], td) == 0.0
                continue
            worst = max(worst, abs(C.cdpp_tail(b["flux"][s], outl[s], td) - ref) / ref)
    assert worst < 1e-10


def test_bls_field_is_found_in_order_by_the_oracle():
    f = C.bls_field()
    step = float(C.BLS_GRID[1] - C.BLS_GRID[0])
    assert len(C.BLS_GRID) == 401 and len(C.BLS_DURATIONS) == 3
    for s in C.row_slices(f["n_off"]):
        found = C.bls_search_oracle(f["time"][s], f["flux"][s], f["flux_err"][s])
        assert abs(found[0][0] - C.BLS_PERIODS[0]) <= step * 1.000001
        assert abs(found[1][0] - C.BLS_PERIODS[1]) <= step * 1.000001
    assert C.near_harmonic(4.2, 2.1, step) and C.near_harmonic(1.05, 2.1, step) and not C.near_harmonic(2.6, 2.1, step)


def test_argument_checks_need_no_device():
    from lightkurve_amd import _capi
    assert _capi.clip_bounds() == (5.0, 5.0, 5)
    assert _capi.clip_bounds(3, sigma_upper=2) == (3.0, 2.0, 5)
    assert _capi.clip_bounds(4.0, 20, None, None) == (20.0, 4.0, -1)
    for bad in (dict(maxiters=-1), dict(sigma=float("nan")), dict(sigma_lower=float("nan"))):
        with pytest.raises(ValueError):
            _capi.clip_bounds(**bad)
    for td in (13.0, 0, -3, True):
        with pytest.raises(ValueError):
            _capi.cdpp_batch(np.ones(10), [0, 10], transit_duration=td)
    with pytest.raises(ValueError):
        _capi.cdpp_batch(np.ones(10), [0, 10], outlier=np.zeros(9, dtype=bool))
