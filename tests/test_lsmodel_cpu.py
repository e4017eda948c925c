"""CPU: ``ls_model_host`` — the pure host restatement of astropy's ``LombScargle.model`` (mle.periodic_fit) and the reference
of the batch kernel (lk_ls_model_batch) — against lightkurve's own ``pg.model`` outputs in the golden file ``pg_misc``, and the
argument checks of the front ends (which run before anything touches a GPU)."""
import numpy as np
import pytest

import lsmodel_cases as cases


def _golden_lc(g):
    keep = ~np.isnan(g["flux"])
    return g["time"][keep], g["flux"][keep]


def _normalised(model):
    return model / np.median(model)          # the reference returns lc.normalize()


def test_ls_model_host_vs_lightkurve(golden):
    """The three golden models at 1e-12: a 3- or 5-column solve over 1200 cadences of a light curve of order one rounds at a
    few 1e-16 (measured 2.2e-16, 2.2e-16, 1.1e-16)."""
    from lightkurve_amd.periodogram import ls_model_host
    g = golden("pg_misc")
    time, flux = _golden_lc(g)
    f_max = float(g["frequency"][np.argmax(g["power"])])
    got = ls_model_host(time, flux, None, f_max)
    assert got["model"].shape == g["model_default"].shape
    assert np.max(np.abs(_normalised(got["model"]) - g["model_default"])) <= 1e-12
    assert got["theta"].shape == (3,) and got["chi2_model"] < got["chi2_ref"]
    fit = ls_model_host(time, flux, None, float(g["model_frequency"]), t_fit=g["tfit"])
    assert fit["model"].shape == g["model_tfit_f"].shape
    assert np.max(np.abs(_normalised(fit["model"]) - g["model_tfit_f"])) <= 1e-12
    two = ls_model_host(time, flux, None, float(g["model_nterms2_frequency"]), nterms=2)
    assert two["theta"].shape == (5,)
    assert np.max(np.abs(_normalised(two["model"]) - g["model_nterms2"])) <= 1e-12


def test_ls_model_host_options_are_a_least_squares_fit():
    """Every fit_mean / center_data combination and flux_err weights: theta is the weighted least-squares solution (the normal
    equations' residual is orthogonal to every column), slot 0 is 0 without fit_mean, chi2_model is what the model leaves."""
    from lightkurve_amd.periodogram import ls_model_host
    rng = np.random.default_rng(11)
    t = 2000.0 + np.sort(rng.uniform(0, 20, 300))
    y = 1 + 5e-3 * np.sin(2 * np.pi * 0.7 * (t - t[0]) + 0.4) + 2e-4 * rng.standard_normal(300)
    dy = rng.uniform(1e-4, 4e-4, 300)
    for fit_mean in (True, False):
        for center in (True, False):
            r = ls_model_host(t, y, dy, 0.7, nterms=2, fit_mean=fit_mean, center_data=center)
            w = dy ** -2.0
            tt = t - t[0]
            cols = [np.ones_like(tt)] if fit_mean else []
            for m in (1, 2):
                cols += [np.sin(2 * np.pi * m * 0.7 * tt), np.cos(2 * np.pi * m * 0.7 * tt)]
            X = np.column_stack(cols)
            resid = y - r["model"]
            assert np.max(np.abs(X.T.dot(w * resid))) <= 1e-7 * np.sum(w * np.abs(y))
            assert fit_mean or r["theta"][0] == 0.0
            assert center or r["y_mean"] == 0.0
            assert np.isclose(r["chi2_model"], np.sum(w * resid ** 2), rtol=1e-12)
            assert np.isclose(r["chi2_ref"], np.sum(w * (y - r["y_mean"]) ** 2), rtol=1e-12)


def test_ls_model_host_singular():
    """A singular fit raises by default (astropy's behaviour); with ``singular="nan"`` it, and a light curve of fewer cadences
    than columns, give NaN everywhere — what the kernel reports as status -1."""
    from lightkurve_amd.periodogram import ls_model_host
    t, y = np.array([10.0, 10.5]), np.array([1.0, 1.01])
    same = np.full(3, 10.0)                              # sin(0) = 0: a zero row and column, singular exactly
    with pytest.raises(np.linalg.LinAlgError):
        ls_model_host(same, np.array([1.0, 1.01, 0.99]), None, 0.8)
    assert np.all(np.isnan(ls_model_host(same, np.array([1.0, 1.01, 0.99]), None, 0.8, singular="nan")["theta"]))
    r = ls_model_host(t, y, None, 0.8, singular="nan")
    assert r["theta"].shape == (3,) and np.all(np.isnan(r["theta"])) and np.all(np.isnan(r["model"]))
    assert np.isnan(r["y_mean"]) and np.isnan(r["chi2_ref"]) and np.isnan(r["chi2_model"])
    r = ls_model_host(t, y, None, 0.8, fit_mean=False, singular="nan")          # two columns, two cadences: determined
    assert np.all(np.isfinite(r["theta"])) and np.max(np.abs(r["model"] - y)) < 1e-12
    r = ls_model_host(t, y, None, 0.8, nterms=2, t_fit=np.linspace(9, 11, 7), singular="nan")
    assert r["theta"].shape == (5,) and r["model"].shape == (7,) and np.all(np.isnan(r["model"]))
    with pytest.raises(ValueError):
        ls_model_host(t, y, None, float("nan"))
    with pytest.raises(ValueError):
        ls_model_host(t, y, None, 0.8, nterms=0)


def test_ls_model_argument_checks():
    """``_capi.ls_model_arguments`` (shared by ``_capi.ls_model_batch``, ``batch.ls_model_batch`` and
    ``DeviceLightCurveBatch.ls_model``): frequency a scalar or one value per target, NaN and <= 0 kept (they mark a skipped
    target); nterms an integer 1 .. 8."""
    from lightkurve_amd import _capi
    f, n = _capi.ls_model_arguments(3, 2.5, 1)
    assert f.shape == (3,) and f.dtype == np.float64 and f.flags.c_contiguous and np.all(f == 2.5) and n == 1
    f, n = _capi.ls_model_arguments(3, [1.0, float("nan"), -2.0], 8)
    assert np.isnan(f[1]) and f[2] == -2.0 and n == 8
    for bad in ([1.0, 2.0], np.ones((3, 1)), np.ones(4)):
        with pytest.raises(ValueError, match="one value per light curve"):
            _capi.ls_model_arguments(3, bad, 1)
    for bad in (0, 9, -1, 1.5):
        with pytest.raises(ValueError, match="nterms"):
            _capi.ls_model_arguments(3, 1.0, bad)


def test_ls_model_dict_amplitude_phase():
    """amplitude / phase per harmonic: theta_sin sin(x) + theta_cos cos(x) = amplitude sin(x + phase)."""
    from lightkurve_amd import _capi
    theta = np.array([[0.25, 3.0, 4.0, 0.0, -2.0], [0.0, -1.0, 0.0, 1.0, 1.0]])
    stats = np.array([[1.0, 9.0, 2.0, 1.0], [np.nan, np.nan, np.nan, -1.0]])
    d = _capi.ls_model_dict([2.0, 3.0], theta, stats)
    assert np.allclose(d["amplitude"], [[5.0, 2.0], [1.0, np.sqrt(2.0)]])
    x = 0.37
    for b in range(2):
        for m in range(2):
            want = theta[b, 1 + 2 * m] * np.sin(x) + theta[b, 2 + 2 * m] * np.cos(x)
            assert np.isclose(d["amplitude"][b, m] * np.sin(x + d["phase"][b, m]), want)
    assert d["offset"][0] == 1.25 and np.isnan(d["offset"][1])
    assert d["status"].tolist() == [1, -1] and d["status"].dtype == np.int64
    assert d["chi2_ref"][0] == 9.0 and d["chi2_model"][0] == 2.0 and d["frequency"].tolist() == [2.0, 3.0]


def test_gpu_test_inputs_meet_their_conditions():
    """The inputs of tests/test_lsmodel_gpu.py, checked where no GPU is needed: every fitted target of the two model batches
    meets ``lsmodel_cases.check_input_condition`` at every option the GPU tests run, and a host prewhitening loop alone (the
    reference's 'fast' periodogram, ``ls_model_host``) finds the injected sinusoids in amplitude order, each within 1 / (2 T),
    with the runner-up grid point at most 0.999 of every round's maximum and the two-sinusoid target below ``PW_MIN_POWER`` in
    round 3 — so the GPU's argmax cannot fall on another grid point."""
    from lightkurve_amd.periodogram import ls_model_host
    from oracle import np_oracle
    for name, targets in cases.model_batches().items():
        assert len(targets) <= 8 and len(set(len(c[0]) for c in targets)) > 1              # ragged, B <= 8
        for t, _y, e, f in targets:
            for nterms, fit_mean, use in [(n, True, False) for n in (1, 2, 3, 8)] + [(n, False, False) for n in (1, 2)] + \
                    [(n, True, True) for n in (1, 2)]:
                if len(t) >= 2 * nterms + int(fit_mean):
                    cases.check_input_condition(t, cases.weights(e, use), f, nterms, fit_mean)
    targets, injected, grid = cases.prewhiten_case()
    assert len(grid) <= 2000
    for b, (t, y) in enumerate(targets):
        cur, found = y.copy(), []
        for r in range(3):
            p = np_oracle.lk_ls_periodogram(t, cur, grid, exact=False)
            top = np.sort(p)[-2:]
            if top[1] < cases.PW_MIN_POWER:
                assert top[1] < 0.5 * cases.PW_MIN_POWER
                break
            assert top[1] > 1.5 * cases.PW_MIN_POWER and top[0] <= 0.999 * top[1], (b, r, top)
            f = float(grid[np.argmax(p)])
            assert abs(f - injected[b][r]) <= 0.5 / (t[-1] - t[0])
            m = ls_model_host(t, cur, None, f)
            cur = cur - (m["model"] - (m["y_mean"] + m["theta"][0]))
            found.append(np.hypot(m["theta"][1], m["theta"][2]))
        assert len(found) == len(injected[b]) == (2 if b == 3 else 3) and found == sorted(found, reverse=True)
