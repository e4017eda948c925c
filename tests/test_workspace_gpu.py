"""GPU: the launchers' device scratch, carved through lk::Scratch plans (lightkurve_amd/csrc/lk_common.hpp).

Every launcher's numbers are already pinned by its own test file; this one covers what those leave open about the scratch:
(a) the smallest shapes at which a conditional buffer of a plan appears or disappears, each against the oracle call and the
tolerance of the entry point's own test; (b) that what an earlier, larger call left in the arena (or a reallocation of the
arena) does not reach a later result — a property, asserted bit for bit; (c) the rebased ('absolute times') path of LS
'fast', whose rebased times live in the launcher's own plan.
"""
import functools

import numpy as np
import pytest

import underfit_cases as U
from lightkurve_amd import _capi, packed, synth
from lightkurve_amd.device import DeviceLightCurveBatch
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-9          # tests/test_ls_gpu.py, test_lschi2_gpu.py, test_lsfast_gpu.py, test_underfit_gpu.py


def relmax(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


def ls_batch(config, B, N, cadence_days=2.0 / 1440.0):
    ts, ys, es = [], [], []
    for b in range(B):
        t, y, e, _ = synth.ls_target(config, b, N, cadence_days)
        ts.append(t - t[0]), ys.append(y), es.append(e)
    return ts, ys, es, np.arange(B + 1) * N


# ------------------------------------------------------------------------------------------------ (a) conditional buffers
@pytest.mark.parametrize("B,N,M", [(1, 4096, 8), (2, 50, 300)])
def test_exact_ls_irregular_grid_with_and_without_cadence_slices(B, N, M):
    """ls_chi2_launch, nterms = 1, explicit frequency array: d_any present, d_freq / d_hot / d_gen null at both shapes.
    B = 1, N = 4096, M = 8: 64 cadence slices, the partial sums d_part present.  B = 2, N = 50, M = 300: one slice, d_part
    null.  Oracle and tolerance of tests/test_ls_gpu.py."""
    ts, ys, es, off = ls_batch(21, B, N)
    T = min(t[-1] for t in ts)
    f = 1.0 / np.linspace(T / 60.0, T / 1.2, M)[::-1]        # irregular (regular in period), >= 1.2 cycles per baseline
    P = _capi.ls_power_batch(np.concatenate(ts), np.concatenate(ys), off, dy=np.concatenate(es), frequency=f,
                             normalization="lk_amplitude")
    for b in range(B):
        d = relmax(P[b], O.ls_power(ts[b], ys[b], es[b], f, fit_mean=True, normalization="lk_amplitude"))
        print("target %d: max |p - ref| / max ref = %.3e" % (b, d))
        assert d < TOL, b


def test_exact_ls_regular_grid_five_terms_makes_its_frequency_array():
    """ls_chi2_launch, nterms = 5 on a regular grid, B = 2, N = 64, M = 40: the launcher writes the grid into d_freq
    (present) and runs the explicit-frequency kernel on d_any; d_part, d_hot, d_gen null.  Oracle and tolerance of
    tests/test_lschi2_gpu.py::test_five_to_eight_terms_run_the_exact_kernel."""
    ts, ys, es, off = ls_batch(22, 2, 64, cadence_days=10.0 / 1440.0)
    T = min(t[-1] for t in ts)
    f0, M = 3.0 / T, 40                                       # f T >= 3 and 5 f below the Nyquist frequency (72 / d)
    df = (13.0 - f0) / M
    f = f0 + df * np.arange(M)
    P = _capi.ls_power_batch(np.concatenate(ts), np.concatenate(ys), off, dy=np.concatenate(es), f0=f0, df=df, M=M,
                             normalization="standard", nterms=5)
    assert np.all(np.isfinite(P))
    for b in range(2):
        d = relmax(P[b], O.ls_power_chi2(ts[b], ys[b], es[b], f, nterms=5, normalization="standard"))
        print("target %d: max |p - ref| / max ref = %.3e" % (b, d))
        assert d < TOL, b


FAST_GRIDS = {20: (4.0, 2.0), 500: (4.0, 0.5)}               # M -> (f0, df): f T >= 1 over the 200 cadences


def fast_peaks_small(M, **kw):
    ts, ys, _es, off = ls_batch(23, 3, 200)
    f0, df = FAST_GRIDS[M]
    return _capi.ls_fast_peaks_batch(np.concatenate(ts), np.concatenate(ys), off, f0=f0, df=df, M=M,
                                     normalization="lk_amplitude", **kw)


@pytest.mark.parametrize("M", [20, 500])
def test_ls_fast_peaks_lds_and_register_path_power_only_and_peaks_only(M):
    """lk_ls_fast_peaks_batch, B = 3, N = 200.  M = 20: FFT grid 128, the in-LDS transforms (lsfast_launch: d_spec present;
    d_grids2, d_tab, d_peaks, d_trel null).  M = 500: grid 4096, the register path (d_grids2 and d_tab present, d_spec null).
    The host pipeline takes its peaks from the spectra (argmax_launch), so d_peaks is null here at both sizes; it is present
    in test_rebased_resident_peaks_equal_the_host_pointer_call below.  Of the pipeline's own plan in the staging arena:
    want_peaks=False leaves d_max / d_arg null, want_power=False keeps every buffer (the spectra stay in HBM); d_scale and
    d_off_all are null in both.  Oracle and tolerance of tests/test_lsfast_gpu.py; peaks as numpy takes them from the spectra."""
    ts, ys, _es, _off = ls_batch(23, 3, 200)
    f0, df = FAST_GRIDS[M]
    P, mx0, am0 = fast_peaks_small(M, want_peaks=False)
    assert mx0 is None and am0 is None
    for b in range(3):
        ref = O.ls_power_fast(ts[b], ys[b], None, f0, df, M, normalization="lk_amplitude")
        ok = np.isfinite(ref)
        assert np.array_equal(ok, np.isfinite(P[b])), b
        d = np.max(np.abs(P[b][ok] - ref[ok])) / np.max(np.abs(ref[ok]))
        print("target %d: max |p - ref| / max ref = %.3e" % (b, d))
        assert d < TOL, b
    P1, mx, am = fast_peaks_small(M, want_power=False)
    assert P1 is None
    assert np.array_equal(mx, np.nanmax(P, axis=1)) and np.array_equal(am, np.nanargmax(P, axis=1))


def regress_problem(rng, n, k, noutl):
    """tests/test_regress_gpu.py: make_problem."""
    t = np.linspace(0, 30, n)
    cols = [np.sin(2 * np.pi * t * rng.uniform(0.05, 3.0) + rng.uniform(0, 6)) for _ in range(k - 1)]
    X = np.column_stack(cols + [np.ones(n)])
    w = rng.normal(0, 1e-3, k)
    w[-1] = 1.0
    err = rng.uniform(0.5, 2.0, n) * 2e-4
    y = X @ w + rng.normal(0, 1, n) * err
    y[rng.integers(0, n, noutl)] += rng.choice([-1, 1], noutl) * 0.01
    cm = np.ones(n, bool)
    cm[n // 3:n // 3 + max(1, n // 50)] = False
    return X, y, err, cm


@functools.lru_cache(maxsize=None)
def regress_small():
    """B = 2, N = 64, K = 3 and the oracle's answer per target, made once (read-only)."""
    rng = np.random.default_rng(24)
    Xs, ys, es, cms = zip(*[regress_problem(rng, 64, 3, 2) for _ in range(2)])
    refs = [O.regression_correct(Xs[b], ys[b], es[b], cms[b]) for b in range(2)]
    return Xs, ys, es, cms, refs


def regress_small_call(**kw):
    Xs, ys, es, cms, _refs = regress_small()
    return _capi.regress_batch(np.vstack(Xs), np.concatenate(ys), [0, 64, 128], err=np.concatenate(es),
                               cadence_mask=np.concatenate(cms), **kw)


def check_cov(cov, ref):
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    d = np.max(np.abs(cov - ref) / scale)
    print("max |cov - ref| / scale = %.3e" % d)
    assert d < 1e-8


@pytest.mark.parametrize("cov", [False, True])
def test_regress_batch_small_with_and_without_covariance(cov):
    """regress_launch, B = 2, N = 64, K = 3: no buffer of the plan is conditional, d_A doubles in size with the covariance
    (K x 2K per target for the inverse).  Oracle and tolerances of tests/test_regress_gpu.py."""
    _Xs, ys, _es, _cms, refs = regress_small()
    r = regress_small_call(return_cov=cov)
    assert ("coefficients_cov" in r) == cov
    for b, ref in enumerate(refs):
        s = slice(64 * b, 64 * b + 64)
        assert np.array_equal(r["outlier_mask"][s], ref["outlier_mask"]), b
        d = np.max(np.abs(r["model"][s] - ref["model"])) / np.std(ys[b])
        print("target %d: max |model - ref| / std = %.3e" % (b, d))
        assert d < 1e-9, b
        assert np.allclose(r["coefficients"][b], ref["coefficients"], rtol=1e-6, atol=1e-9), b
        if cov:
            check_cov(r["coefficients_cov"][b], ref["coefficients_cov"])


@functools.lru_cache(maxsize=None)
def shared_small():
    """B = 17, N = 300, K = 2 (tests/test_regress_shared_gpu.py: make_shared) and the oracle's answers, made once."""
    B, N, K = 17, 300, 2
    t = np.linspace(0, 30, N)
    rng = np.random.default_rng(25)
    X = np.column_stack([np.sin(2 * np.pi * t * rng.uniform(0.05, 3.0) + rng.uniform(0, 6)), np.ones(N)])
    W = rng.normal(0, 1e-3, (B, K))
    W[:, -1] = 1.0
    err = rng.uniform(0.5, 2.0, (B, N)) * 2e-4
    y = W @ X.T + rng.normal(0, 1, (B, N)) * err
    cm = np.ones((B, N), bool)
    for b in range(B):
        y[b, rng.integers(0, N, 6)] += rng.choice([-1, 1], 6) * 0.01
        lo = int(rng.integers(0, N - N // 50 + 1))
        cm[b, lo:lo + N // 50] = False
    refs = [O.regression_correct(X, y[b], err[b], cm[b]) for b in range(B)]
    for a in (X, y, err, cm):
        a.setflags(write=False)
    return X, y, err, cm, refs


@pytest.mark.parametrize("cov", [False, True])
def test_regress_shared_two_target_tiles_two_cadence_slices(cov):
    """regress_shared_launch, B = 17, N = 300, K = 2: two tiles of 16 targets (the second holds one), two cadence slices in
    d_part; no buffer of the plan is conditional, d_A doubles with the covariance.  Oracle and tolerances of
    tests/test_regress_shared_gpu.py."""
    X, y, err, cm, refs = shared_small()
    r = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, want_cov=cov)
    assert ("coefficients_cov" in r) == cov
    worst = 0.0
    for b, ref in enumerate(refs):
        assert np.array_equal(r["outlier_mask"][b], ref["outlier_mask"]), b
        d = np.max(np.abs(r["model"][b] - ref["model"])) / np.std(y[b])
        worst = max(worst, d)
        assert d < 1e-9, (b, d)
        assert np.allclose(r["coefficients"][b], ref["coefficients"], rtol=1e-6, atol=1e-9), b
        if cov:
            check_cov(r["coefficients_cov"][b], ref["coefficients_cov"])
    print("max |model - ref| / std = %.3e" % worst)


def test_underfit_without_neighbours_has_zero_length_buffers():
    """lk_underfit_neighbors_batch, M = 0 neighbours, B = 2, N = 8: the neighbour lists and the correlations are zero-length
    buffers of the host-pointer call (they still get non-null device pointers); the launcher's d_z and d_g are present, the
    prepare kernel is skipped.  Mirror and tolerance of tests/test_underfit_gpu.py; no neighbours is a metric of exactly 1."""
    f = U.field(26, 2, 8, 1)
    none = np.zeros((2, 0), dtype=np.int32)
    r = _capi.underfit_neighbors_batch(f["y"], none)
    ref_m, _ref_c = U.mirror(f["y"], none)
    assert r["correlations"].shape == (2, 0) and np.all(r["metric"] == 1.0)
    assert np.max(np.abs(r["metric"] - ref_m)) < TOL


# ------------------------------------------------------------------------------------------------ (b) arena history
def fold_small():
    rng = np.random.default_rng(27)
    sizes = [5, 300]
    ts = [np.sort(rng.uniform(0, 30, n)) for n in sizes]
    fl = [rng.normal(1, 1e-3, n) for n in sizes]
    periods, epochs = np.array([1.7, 4.3]), np.array([-2.0, 3.5])
    ph, order, (flux,) = _capi.fold_batch(np.concatenate(ts), [0, 5, 305], periods, epochs, epoch_phase=0.1,
                                          columns=(np.concatenate(fl),))
    return (ph, order, flux), (ts, fl, periods, epochs)


def test_a_larger_call_in_between_does_not_change_a_small_result():
    """Small call, a call of another entry point whose scratch is about 8 x larger or more (savgol_trend_batch, B = 4,
    N = 20 000: the arena is freed and reallocated unless an earlier test of the same process already grew it), the small
    call again: bit-identical, for LS 'fast' peaks, regress_batch and fold_batch.  The small LS and regression results are
    the ones checked against the oracle above; the fold is checked here (tests/test_fold_gpu.py: bit-identical phases, the
    stable argsort)."""
    h = _capi.Handle.get(0)

    def smalls():
        P, mx, am = fast_peaks_small(500)
        r = regress_small_call(return_cov=True)
        fold, _ = fold_small()
        return [P, mx, am, r["coefficients"], r["model"], r["outlier_mask"], r["coefficients_cov"], *fold]

    first = smalls()
    before = h.workspace_bytes()
    t, y, _e, off = synth.ls_batch(28, 4, 20000)
    trend = _capi.savgol_trend_batch(t, y, off, window_length=101)
    assert trend.shape == t.shape and np.all(np.isfinite(trend))
    print("workspace bytes: %d before the larger call, %d after" % (before, h.workspace_bytes()))
    second = smalls()
    for k, (a, b) in enumerate(zip(first, second)):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
    (ph, order, flux), (ts, fl, periods, epochs) = fold_small()
    for b, sl in enumerate((slice(0, 5), slice(5, 305))):
        rph, rorder, _ = O.fold(ts[b], periods[b], epochs[b], epoch_phase=0.1)
        assert np.array_equal(ph[sl], rph) and np.array_equal(order[sl], rorder) and np.array_equal(flux[sl], fl[b][rorder])


# ------------------------------------------------------------------------------------------------ (c) the rebased path
def test_rebased_resident_peaks_equal_the_host_pointer_call():
    """B = 3, N = 200, times near 2 457 000 d.  The resident batch calls lk_ls_fast_peaks_lc_batch_dev: lsfast_launch rebases
    into d_trel of its own plan and takes the peaks from the fused kernel's partials (d_trel and d_peaks present).  The
    host-pointer call (absolute_time=True) rebases its chunk in place and takes the peaks from the spectra.  Same kernels on
    the same numbers: equal bit for bit.  (tests/test_device_batch_gpu.py compares the two only through LightCurveBatch, on
    normalised light curves of other sizes.)"""
    ts, ys, _es, off = ls_batch(23, 3, 200)
    t_abs = np.concatenate([t + 2457000.0 + 3.25 * b for b, t in enumerate(ts)])
    y = np.concatenate(ys)
    f = 4.0 + 0.5 * np.arange(500)
    dev = DeviceLightCurveBatch.from_arrays(t_abs, y, None, off)
    pk = dev.to_periodogram_peaks(f)
    plan = packed.ls_grid_plan(f, "amplitude", None, None, "fast", 1)
    P, mx, am = _capi.ls_fast_peaks_batch(t_abs, y, off, f0=float(plan.f_day[0]), df=float(plan.f_day[1] - plan.f_day[0]),
                                          M=len(f), normalization=plan.norm, absolute_time=True)
    assert np.all(np.isfinite(mx)) and np.array_equal(mx, np.nanmax(P, axis=1))
    assert pk.shape == (3, 2) and np.array_equal(pk[:, 0], mx) and np.array_equal(pk[:, 1], am.astype(np.float64))
