"""GPU: regression of a batch on ONE shared design matrix (lk_regress_shared_batch*, DeviceLightCurveBatch.regression_correct /
.cbv_correct) against the numpy oracle per target and the reference golden `cbv_ridge`.  Tolerances are the house ones of
test_regress_gpu.py: outlier masks identical; model within 1e-9 * std(flux) absolute; coefficients rtol 1e-6, atol 1e-9.
The four generated configurations keep every residual at least 7e-3 standard deviations away from a clip bound in the oracle,
so a kernel that is right to 1e-9 cannot flip a mask.  Shapes: partial target tiles (B not a multiple of 16), partial
32-cadence stages, two to nine cadence slices per target, pair counts that do not fill the last 16-column tile, K = 64 = the
bound of the path."""
import numpy as np
import pytest

from lightkurve_amd import LightCurveBatch, _capi
from lightkurve_amd.device import DeviceBuffer, DeviceLightCurveBatch
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
KMAX = 64                     # SH_KMAX of regress.hip


def make_shared(seed, B, N, K, noutl=6):
    t = np.linspace(0, 30, N)
    rng = np.random.default_rng(seed)
    cols = [np.sin(2 * np.pi * t * rng.uniform(0.05, 3.0) + rng.uniform(0, 6)) for _ in range(K - 1)]
    X = np.column_stack(cols + [np.ones(N)])
    W = rng.normal(0, 1e-3, (B, K))
    W[:, -1] = 1.0
    err = rng.uniform(0.5, 2.0, (B, N)) * 2e-4
    y = W @ X.T + rng.normal(0, 1, (B, N)) * err
    cm = np.ones((B, N), bool)
    for b in range(B):
        y[b, rng.integers(0, N, noutl)] += rng.choice([-1, 1], noutl) * 0.01
        lo = int(rng.integers(0, N - N // 50 + 1))
        cm[b, lo:lo + N // 50] = False
    return X, y, err, cm


_CACHE = {}


def problem(seed, B, N, K):
    """The generated batch and the oracle's answer per target, computed once and shared (read-only) by the tests."""
    key = (seed, B, N, K)
    if key not in _CACHE:
        X, y, err, cm = make_shared(seed, B, N, K)
        refs = [O.regression_correct(X, y[b], err[b], cm[b]) for b in range(B)]
        for a in (X, y, err, cm):
            a.setflags(write=False)
        _CACHE[key] = (X, y, err, cm, refs)
    return _CACHE[key]


def check(r, y, refs, cov=False):
    for b, ref in enumerate(refs):
        assert np.array_equal(r["outlier_mask"][b], ref["outlier_mask"]), b
        dev = np.max(np.abs(r["model"][b] - ref["model"])) / np.std(y[b])
        assert dev < 1e-9, (b, dev)
        assert np.allclose(r["coefficients"][b], ref["coefficients"], rtol=1e-6, atol=1e-9), b


CONFIGS = [(11, 37, 1003, 17), (12, 19, 517, 3), (13, 21, 2050, 33), (14, 17, 700, 64)]


@pytest.mark.parametrize("seed,B,N,K", CONFIGS)
def test_generated_batches_vs_oracle(seed, B, N, K):
    X, y, err, cm, refs = problem(seed, B, N, K)
    r = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm)
    assert r["model"].shape == (B, N) and r["outlier_mask"].shape == (B, N) and r["coefficients"].shape == (B, K)
    print("clipped per target:", sorted(set(int(ref["outlier_mask"].sum()) for ref in refs)),
          "max |model - ref| / std:", max(np.max(np.abs(r["model"][b] - refs[b]["model"])) / np.std(y[b]) for b in range(B)))
    check(r, y, refs)


def test_one_target_five_cadences_one_column():
    rng = np.random.default_rng(1)
    X = np.ones((5, 1))
    y = 3.0 + rng.normal(0, 1e-3, (1, 5))
    err = np.full((1, 5), 1e-3)
    r = _capi.regress_shared_batch(X, y, err=err)
    check(r, y, [O.regression_correct(X, y[0], err[0])])


def test_without_errors():
    X, y, err, cm, _ = problem(12, 19, 517, 3)
    r = _capi.regress_shared_batch(X, y, cadence_mask=cm)
    check(r, y, [O.regression_correct(X, y[b], None, cm[b]) for b in range(len(y))])


def test_priors_on_every_second_column_different_per_target():
    X, y, err, cm, _ = problem(11, 37, 1003, 17)
    B, K = len(y), X.shape[1]
    rng = np.random.default_rng(111)
    mu = np.zeros((B, K))
    mu[:, ::2] = rng.normal(0, 1e-3, (B, (K + 1) // 2))
    sg = np.full((B, K), np.inf)
    sg[:, ::2] = 0.05
    r = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, prior_mu=mu, prior_sigma=sg)
    check(r, y, [O.regression_correct(X, y[b], err[b], cm[b], mu[b], sg[b]) for b in range(B)])
    with pytest.raises(ValueError, match="both"):
        _capi.regress_shared_batch(X, y, err=err, prior_mu=mu)


def test_one_column_past_the_bound_is_refused_and_names_the_other_entry_point():
    rng = np.random.default_rng(2)
    X = rng.normal(0, 1, (200, KMAX + 1))
    y = rng.normal(1, 1e-3, (3, 200))
    with pytest.raises(ValueError, match="lk_regress_batch") as ei:
        _capi.regress_shared_batch(X, y)
    assert str(KMAX) in str(ei.value)


def test_target_with_an_empty_cadence_mask_returns_its_prior():
    X, y, err, cm, refs = problem(12, 19, 517, 3)
    B, K = len(y), X.shape[1]
    cm = cm.copy()
    cm[4] = False
    mu = np.tile(np.array([0.5, -0.25, 1.0]), (B, 1))
    sg = np.full((B, K), 10.0)
    r = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, prior_mu=mu, prior_sigma=sg)
    assert np.allclose(r["coefficients"][4], mu[4], rtol=1e-12, atol=0)
    others = [b for b in range(B) if b != 4]
    ref = [O.regression_correct(X, y[b], err[b], cm[b], mu[b], sg[b]) for b in others]
    check({k: v[others] for k, v in r.items()}, y[others], ref)


def test_a_clip_that_removes_300_of_9000_cadences_changes_the_next_fit():
    """As the delta-Gram test of test_regress_gpu.py: 3.3 % of one target's cadences raised by 1.0 are all clipped by the
    first pass, so passes 2.. fit a different mask (here: the Gram is recomputed in full from the new outlier bytes)."""
    N, K = 9000, 40
    X, y, err, cm = make_shared(5, 3, N, K, noutl=0)
    rng = np.random.default_rng(55)
    y[0, rng.choice(N, 300, replace=False)] += 1.0
    r = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm)
    refs = [O.regression_correct(X, y[b], err[b], cm[b]) for b in range(3)]
    assert refs[0]["outlier_mask"].sum() >= 300
    check(r, y, refs)


def test_non_finite_flux_or_a_zero_error_is_an_error():
    X, y, err, cm, _ = problem(12, 19, 517, 3)
    bad = y.copy()
    bad[7, 100] = np.nan
    with pytest.raises(ValueError, match="NaNs in the flux"):
        _capi.regress_shared_batch(X, bad, err=err, cadence_mask=cm)
    bad = err.copy()
    bad[18, 516] = 0.0
    with pytest.raises(ValueError, match="flux errors"):
        _capi.regress_shared_batch(X, y, err=bad, cadence_mask=cm)
    dev = DeviceLightCurveBatch.from_arrays(np.tile(np.linspace(0, 30, 517), 19), y.ravel(), bad.ravel(), np.arange(20) * 517)
    with pytest.raises(ValueError, match="flux errors"):
        dev.regression_correct(X)


def _golden_checks(g, tag, outl, corrected, coef):
    assert np.array_equal(outl, g["outlier_" + tag]), tag
    assert np.max(np.abs(corrected - g["corrected_" + tag])) <= 1e-9 * np.max(np.abs(g["corrected_" + tag])), tag
    assert np.allclose(coef, g["coefficients_" + tag], rtol=1e-7, atol=1e-9 * np.abs(g["coefficients_" + tag]).max()), tag


def test_reference_golden_three_ridge_widths_in_one_batch(golden):
    """Three copies of the golden light curve carry the three alphas as per-target prior widths over the shared
    [cbvs[:, :8] | 1]; tolerances of test_cbv_gaussian_prior_golden."""
    g = golden("cbv_ridge")
    tags = ("weak", "ridge", "none")
    X = np.column_stack([g["cbvs"][:, :8], np.ones(len(g["time"]))])
    sig = [np.inf if float(g["alpha_" + t]) == 0.0 else np.median(g["flux_err"]) / np.sqrt(abs(float(g["alpha_" + t]))) for t in tags]
    y, err, cm = (np.tile(g[k], (3, 1)) for k in ("flux", "flux_err", "cadence_mask"))
    r = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, prior_mu=np.zeros((3, 9)),
                                   prior_sigma=np.repeat(np.array(sig)[:, None], 9, axis=1))
    for b, tag in enumerate(tags):
        _golden_checks(g, tag, r["outlier_mask"][b], y[b] - r["model"][b], r["coefficients"][b])


def test_reference_golden_through_cbv_correct(golden):
    g = golden("cbv_ridge")
    n = len(g["time"])
    B = 3                    # identical copies per alpha: every target must give the golden
    dev = DeviceLightCurveBatch.from_arrays(np.tile(g["time"], B), np.tile(g["flux"], B), np.tile(g["flux_err"], B),
                                            np.arange(B + 1) * n)
    cm = np.tile(g["cadence_mask"], (B, 1))
    for tag in ("weak", "ridge", "none"):
        corrected, outl, coef = dev.cbv_correct(g["cbvs"], alpha=float(g["alpha_" + tag]), cadence_mask=cm, to_host=True)
        for b in range(B):
            _golden_checks(g, tag, outl[b], corrected[b], coef[b])


def test_coefficient_covariance_vs_oracle():
    X, y, err, cm, refs = problem(11, 37, 1003, 17)
    r = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, want_cov=True)
    check(r, y, refs)
    for b, o in enumerate(refs):
        ref = o["coefficients_cov"]
        scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
        assert np.max(np.abs(r["coefficients_cov"][b] - ref) / scale) < 1e-8, b


def test_bitwise_reproducible_and_independent_of_the_batch_around_a_target():
    X, y, err, cm, _ = problem(13, 21, 2050, 33)
    B = len(y)
    a = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, want_cov=True)
    b = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, want_cov=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # the same 21 targets at other places of a batch of 40 (other tile mates, another grid): same bits
    X2, y2, err2, cm2 = make_shared(131, 40, 2050, 33)
    where = np.r_[np.arange(3, 40, 2), 0, 38][:B]
    y2[where], err2[where], cm2[where] = y, err, cm
    c = _capi.regress_shared_batch(X, y2, err=err2, cadence_mask=cm2, want_cov=True)
    for k in a:
        assert np.array_equal(a[k], c[k][where]), k


def test_regression_correct_resident_equals_the_host_pointer_call():
    from lightkurve_amd.correctors import DesignMatrix, DesignMatrixCollection
    X, y, err, cm, _ = problem(12, 19, 517, 3)
    B, N = y.shape
    t = np.tile(np.linspace(0, 30, N), B)
    dev = DeviceLightCurveBatch.from_arrays(t, y.ravel(), err.ravel(), np.arange(B + 1) * N)
    dmc = DesignMatrixCollection([DesignMatrix(X[:, :2], name="sines", prior_mu=[0.0, 1e-3], prior_sigma=[0.05, np.inf]),
                                  DesignMatrix(X[:, 2:], name="offset")], validate_rank=False)
    ref = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, prior_mu=dmc.prior_mu, prior_sigma=dmc.prior_sigma)
    corrected, outl, coef = dev.regression_correct(dmc, cadence_mask=cm, to_host=True)
    assert np.array_equal(corrected, y - ref["model"]) and np.array_equal(outl, ref["outlier_mask"])
    assert np.array_equal(coef, ref["coefficients"])
    out, d_outl, d_w = dev.regression_correct(dmc, cadence_mask=cm)
    assert isinstance(d_outl, DeviceBuffer) and isinstance(d_w, DeviceBuffer)
    assert np.array_equal(out.flux_host().reshape(B, N), corrected) and np.array_equal(out.flux_err_host(), err.ravel())
    assert np.array_equal(d_w.download(np.float64, B * 3).reshape(B, 3), coef)
    assert np.array_equal(d_outl.download(np.uint8, B * N).reshape(B, N).astype(bool), outl)


def test_cbv_correct_then_flatten_resident_equals_the_staged_chain():
    X, y, err, cm, _ = problem(11, 37, 1003, 17)
    B, N = y.shape
    t = np.tile(np.linspace(0, 30, N), B)
    off = np.arange(B + 1) * N
    cbvs = X[:, :16]
    dev = DeviceLightCurveBatch.from_arrays(t, y.ravel(), err.ravel(), off)
    flat = dev.cbv_correct(cbvs, cbv_indices="ALL", alpha=0.5, cadence_mask=cm, to_host=False)[0].flatten(101).to_host()
    corrected, _, _ = dev.cbv_correct(cbvs, cbv_indices="ALL", alpha=0.5, cadence_mask=cm, to_host=True)
    # the ridge width taken on the device is numpy's median(flux_err_b) / sqrt(|alpha|), bit for bit
    sg = np.repeat((np.median(err, axis=1) / np.sqrt(0.5))[:, None], 17, axis=1)
    ref = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, prior_mu=np.zeros((B, 17)), prior_sigma=sg)
    assert np.array_equal(corrected, y - ref["model"])
    host = LightCurveBatch(t, corrected.ravel(), err.ravel(), off)
    trend = host.flatten_trend(window_length=101)
    assert np.array_equal(flat.flux, host.flux / trend, equal_nan=True)
    assert np.array_equal(flat.flux_err, host.flux_err / trend, equal_nan=True)
    assert np.array_equal(flat.time, t)
