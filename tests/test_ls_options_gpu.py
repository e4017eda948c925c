"""astropy's fit_mean / center_data / normalization options on every Lomb-Scargle path of the batch API.

The launchers form ``center = fit_mean || center_data``; the uncentred branch of ls_prep_kernel / lsf_prep_kernel
(fit_mean=False, center_data=False: ybar = 0, YY = sum w y^2) and normalization="standard" on the one-term 'fast' path (the only
consumer of FastStats::YY there, and astropy's own default) are compared here with the oracle for every combination of
(fit_mean, center_data) x dy None / array x {standard, psd, lk_amplitude}, on one ragged batch (n = 257, 1000, 640) whose means
matter: two targets near 1.0, one at 3e3.

References: O.ls_power (C), O.ls_power_chi2, O.ls_power_fast, O.ls_power_fastchi2 — never another path of the library.
Tolerance: max |gpu - ref| <= 1e-9 max |ref| per target on the band f T >= nterms with T = t.max() - t.min() (a fit of nterms
harmonics and a mean needs its lowest harmonic to complete a cycle and the highest one nterms of them; below that X^T X is close
to singular and 1e-9 is not the reference's own precision), identical finite / NaN pattern there.  The worst relative error of
every case is printed.

The conditioning cases put the first cadence D = 1e4 and 1e6 sigma off with a matching error bar: sum w (y - ybar)^2 is then
~sigma^2 while the sums about y[0] are ~D^2, so a one-sweep shifted formula for YY loses log10(D^2 / sigma^2) digits."""
import functools
import itertools

import numpy as np
import pytest

from lightkurve_amd import _capi
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-9
NORMS = ("standard", "psd", "lk_amplitude")
FMCD = [(True, True), (True, False), (False, True), (False, False)]
CASES = [(fm, cd, use_dy) for (fm, cd), use_dy in itertools.product(FMCD, (False, True))]
CASE_IDS = ["%s%s-%s" % ("FT"[fm], "FT"[cd], "dy" if d else "nody") for fm, cd, d in CASES]

NS = (257, 1000, 640)
LEVEL = (1.0, 3e3, 1.0)
SPAN = 27.0
M_EXACT, F0_EXACT, DF_EXACT = 333, 0.02, 0.0301             # 333: no multiple of a tile of frequencies
M_FAST, F0_FAST, DF_FAST = 3000, 0.013, 0.0417


@functools.lru_cache(maxsize=None)
def batch():
    ts, ys, es = [], [], []
    for b, (n, level) in enumerate(zip(NS, LEVEL)):
        rng = np.random.default_rng(3100 + b)
        t = np.sort(rng.uniform(0.0, SPAN, n))
        t[0] = 0.0
        y = level * (1.0 + 5e-3 * np.sin(2 * np.pi * (1.7 + 2.1 * b) * t + 0.3 * b) + rng.normal(0, 5e-4, n))
        e = level * 5e-4 * rng.uniform(0.5, 3.0, n)
        ts.append(t), ys.append(y), es.append(e)
    off = np.zeros(len(NS) + 1, dtype=np.int64)
    off[1:] = np.cumsum(NS)
    return ts, ys, es, np.concatenate(ts), np.concatenate(ys), np.concatenate(es), off


def uneven_grid():
    rng = np.random.default_rng(3200)
    return F0_EXACT + DF_EXACT * (np.arange(M_EXACT) + rng.uniform(-0.4, 0.4, M_EXACT))


def rel_err(got, ref, fr, t, nterms, label):
    cond = fr * (t.max() - t.min()) >= nterms
    assert cond.sum() > len(fr) // 2
    assert np.array_equal(np.isfinite(ref[cond]), np.isfinite(got[cond])), label
    ok = cond & np.isfinite(ref)
    err = np.max(np.abs(got[ok] - ref[ok])) / np.max(np.abs(ref[ok]))
    print("%s: rel err %.3e" % (label, err))
    return err


def exact_ref(t, y, e, fr, nterms, fm, cd, norm):
    if nterms == 1:
        return O.ls_power(t, y, e, fr, fit_mean=fm, center_data=cd, normalization=norm)
    return O.ls_power_chi2(t, y, e, fr, nterms=nterms, fit_mean=fm, center_data=cd, normalization=norm)


def check_exact(fm, cd, use_dy, fr, grid_kw, what):
    ts, ys, es, t, y, e, off = batch()
    worst = {}
    for nterms, norm in itertools.product((1, 2, 5), NORMS):
        P = _capi.ls_power_batch(t, y, off, dy=e if use_dy else None, fit_mean=fm, center_data=cd, normalization=norm,
                                 nterms=nterms, **grid_kw)
        assert P.shape == (len(NS), len(fr))
        for b in range(len(NS)):
            ref = exact_ref(ts[b], ys[b], es[b] if use_dy else None, fr, nterms, fm, cd, norm)
            label = "%s fit_mean %d center_data %d dy %d nterms %d %s target %d" % (what, fm, cd, use_dy, nterms, norm, b)
            worst[label] = rel_err(P[b], ref, fr, ts[b], nterms, label)
    bad = {k: v for k, v in worst.items() if not v <= TOL}
    assert not bad, bad


@pytest.mark.parametrize("fm,cd,use_dy", CASES, ids=CASE_IDS)
def test_exact_regular_grid(fm, cd, use_dy):
    fr = F0_EXACT + DF_EXACT * np.arange(M_EXACT)
    check_exact(fm, cd, use_dy, fr, dict(f0=F0_EXACT, df=DF_EXACT, M=M_EXACT), "exact regular")


@pytest.mark.parametrize("fm,cd,use_dy", CASES, ids=CASE_IDS)
def test_exact_frequency_array(fm, cd, use_dy):
    fr = uneven_grid()
    check_exact(fm, cd, use_dy, fr, dict(frequency=fr), "exact frequency=")


@pytest.mark.parametrize("fm,cd", [(False, False), (False, True)], ids=["FF", "FT"])
@pytest.mark.parametrize("norm", NORMS)
def test_exact_cadence_sliced_single_target(fm, cd, norm):
    """B = 1, 20 000 cadences x 2000 uneven frequencies: ls_any_kernel in slices of the cadences; every 50th frequency."""
    rng = np.random.default_rng(3300)
    n = 20000
    t = np.sort(rng.uniform(0.0, 80.0, n))
    t[0] = 0.0
    y = 3e3 * (1.0 + 5e-3 * np.sin(2 * np.pi * 0.77 * t) + rng.normal(0, 5e-4, n))
    e = 3e3 * 5e-4 * rng.uniform(0.5, 3.0, n)
    f = 1.0 / np.linspace(0.3, 40.0, 2000)[::-1]
    p = _capi.ls_power_batch(t, y, [0, n], dy=e, frequency=f, fit_mean=fm, center_data=cd, normalization=norm)[0]
    ref = O.ls_power(t, y, e, f[::50], fit_mean=fm, center_data=cd, normalization=norm)
    err = rel_err(p[::50], ref, f[::50], t, 1, "exact sliced fit_mean %d center_data %d %s" % (fm, cd, norm))
    assert err <= TOL, err


@pytest.mark.parametrize("fm,cd,use_dy", CASES, ids=CASE_IDS)
def test_fast_and_fastchi2(fm, cd, use_dy):
    """ls_fast_batch nterms 1, 2, 3 and ls_fast_peaks_batch, every normalisation on the whole grid."""
    ts, ys, es, t, y, e, off = batch()
    fr = F0_FAST + DF_FAST * np.arange(M_FAST)
    d = e if use_dy else None
    worst = {}
    for norm in NORMS:
        pw, mx, am = _capi.ls_fast_peaks_batch(t, y, off, dy=d, f0=F0_FAST, df=DF_FAST, M=M_FAST, fit_mean=fm,
                                               center_data=cd, normalization=norm)
        assert np.array_equal(mx, np.nanmax(pw, axis=1)) and np.array_equal(am, np.nanargmax(pw, axis=1))
        P1 = _capi.ls_fast_batch(t, y, off, dy=d, f0=F0_FAST, df=DF_FAST, M=M_FAST, fit_mean=fm, center_data=cd,
                                 normalization=norm)
        assert np.array_equal(pw, P1, equal_nan=True)
        for b in range(len(NS)):
            ref = O.ls_power_fast(ts[b], ys[b], es[b] if use_dy else None, F0_FAST, DF_FAST, M_FAST, normalization=norm,
                                  fit_mean=fm, center_data=cd)
            label = "fast fit_mean %d center_data %d dy %d %s target %d" % (fm, cd, use_dy, norm, b)
            worst[label] = rel_err(P1[b], ref, fr, ts[b], 1, label)
        for nterms in (2, 3):
            P = _capi.ls_fast_batch(t, y, off, dy=d, f0=F0_FAST, df=DF_FAST, M=M_FAST, fit_mean=fm, center_data=cd,
                                    normalization=norm, nterms=nterms)
            for b in range(len(NS)):
                ref = O.ls_power_fastchi2(ts[b], ys[b], es[b] if use_dy else None, F0_FAST, DF_FAST, M_FAST, nterms=nterms,
                                          fit_mean=fm, center_data=cd, normalization=norm)
                label = "fastchi2 fit_mean %d center_data %d dy %d nterms %d %s target %d" % (fm, cd, use_dy, nterms, norm, b)
                worst[label] = rel_err(P[b], ref, fr, ts[b], nterms, label)
    bad = {k: v for k, v in worst.items() if not v <= TOL}
    assert not bad, bad


@pytest.mark.parametrize("use_dy", (False, True), ids=["nody", "dy"])
def test_fit_mean_makes_center_data_irrelevant_bit_for_bit(use_dy):
    ts, ys, es, t, y, e, off = batch()
    d = e if use_dy else None
    fr = uneven_grid()
    calls = []
    for norm in NORMS:
        for nterms in (1, 2, 5):
            calls.append(lambda cd, n=norm, k=nterms: _capi.ls_power_batch(
                t, y, off, dy=d, f0=F0_EXACT, df=DF_EXACT, M=M_EXACT, center_data=cd, normalization=n, nterms=k))
            calls.append(lambda cd, n=norm, k=nterms: _capi.ls_power_batch(
                t, y, off, dy=d, frequency=fr, center_data=cd, normalization=n, nterms=k))
        for nterms in (1, 2, 3):
            calls.append(lambda cd, n=norm, k=nterms: _capi.ls_fast_batch(
                t, y, off, dy=d, f0=F0_FAST, df=DF_FAST, M=M_FAST, center_data=cd, normalization=n, nterms=k))
        calls.append(lambda cd, n=norm: np.column_stack([x.astype(np.float64) for x in _capi.ls_fast_peaks_batch(
            t, y, off, dy=d, f0=F0_FAST, df=DF_FAST, M=M_FAST, center_data=cd, normalization=n, want_power=False)[1:]]))
    for k, call in enumerate(calls):
        a, b = call(True), call(False)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), k


# ------------------------------------------------------------------------------------ conditioning of YY ('standard')
def conditioning_target(D, with_dy):
    rng = np.random.default_rng(3400)
    n, sigma = 3000, 1e-3
    t = np.sort(rng.uniform(0.0, SPAN, n))
    t[0] = 0.0
    y = 1.0 + 5e-3 * np.sin(2 * np.pi * 2.3 * t + 0.7) + rng.normal(0, sigma, n)
    y[0] += D
    e = None
    if with_dy:
        e = np.full(n, sigma)
        e[0] = D
    return t, y, e


@pytest.mark.parametrize("D,with_dy", [(10.0, True), (1000.0, True), (10.0, False)], ids=["D1e4sigma", "D1e6sigma", "nody_D10"])
@pytest.mark.parametrize("nterms", (1, 2))
def test_standard_normalisation_with_a_far_first_cadence(D, with_dy, nterms):
    t, y, e = conditioning_target(D, with_dy)
    off = [0, len(t)]
    fr = F0_FAST + DF_FAST * np.arange(M_FAST)
    got = _capi.ls_fast_batch(t, y, off, dy=e, f0=F0_FAST, df=DF_FAST, M=M_FAST, normalization="standard", nterms=nterms)[0]
    if nterms == 1:
        ref = O.ls_power_fast(t, y, e, F0_FAST, DF_FAST, M_FAST, normalization="standard")
    else:
        ref = O.ls_power_fastchi2(t, y, e, F0_FAST, DF_FAST, M_FAST, nterms=nterms, normalization="standard")
    label = "standard, first cadence %g off, dy %d, nterms %d" % (D, with_dy, nterms)
    err = rel_err(got, ref, fr, t, nterms, label + " vs port")
    exact = _capi.ls_power_batch(t, y, off, dy=e, f0=F0_FAST, df=DF_FAST, M=M_FAST, normalization="standard", nterms=nterms)[0]
    band = np.isfinite(got) & (fr * t.max() >= nterms)
    gap = np.max(np.abs(got[band] - exact[band])) / np.nanmax(exact)
    print("%s: fast vs exact %.3e of the peak" % (label, gap))
    assert err <= TOL, (label, err)
    assert gap < 5e-3, (label, gap)
