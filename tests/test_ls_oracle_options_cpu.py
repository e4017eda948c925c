"""The option-aware numpy port of astropy's 'fast' Lomb-Scargle (oracle.np_oracle.ls_power_fast: fit_mean, center_data,
oversampling, normalization="standard") against an independent restatement of the same quantity from the same extirpolated
sums: ls_power_fastchi2(nterms=1) solves the normal equations where ls_power_fast evaluates the closed form.  All 16
combinations of fit_mean x center_data x dy None / array x {psd, standard}, on f T >= 1 (below one cycle per baseline both
forms cancel).  The two agree to a few 1e-15 of the largest power; the bound is 1e-12 — a larger gap is a wrong restatement,
not rounding.  With the default arguments the function must return the bits it returned before it took options (every
golden of test_oracle_golden.py pins those), and ls_power_fastchi2's ``idx`` must pick out the full result's values."""
import itertools

import numpy as np
import pytest

from oracle import np_oracle as O

N, M, F0, DF = 1500, 4000, 0.004, 0.004
TOL = 1e-12


def target():
    rng = np.random.default_rng(42)
    t = np.sort(rng.uniform(0.0, 27.0, N))
    t[0] = 0.0
    y = 1.0 + 5e-3 * np.sin(2 * np.pi * 3.3 * t + 0.4) + rng.normal(0, 5e-4, N)
    dy = 5e-4 * rng.uniform(0.5, 2.0, N)
    return t, y, dy


def fast_before_options(t, y, dy, f0, df, nf, normalization="psd", lk_scale=1.0):
    """Verbatim copy of ls_power_fast's body before it took fit_mean / center_data / oversampling / 'standard'."""
    t, y = np.asarray(t, float), np.asarray(y, float)
    w = np.ones_like(t) if dy is None else np.broadcast_to(np.asarray(dy, float), t.shape) ** -2.0
    wsum = w.sum()
    w = w / wsum
    y = y - np.dot(w, y)
    Sh, Ch = O._trig_sum_fft(t, w * y, df, nf, f0)
    S2, C2 = O._trig_sum_fft(t, w, df, nf, f0, freq_factor=2)
    S, C = O._trig_sum_fft(t, w, df, nf, f0)
    tan2 = (S2 - 2 * S * C) / (C2 - (C * C - S * S))
    S2w = tan2 / np.sqrt(1 + tan2 * tan2)
    C2w = 1 / np.sqrt(1 + tan2 * tan2)
    Cw = np.sqrt(0.5) * np.sqrt(1 + C2w)
    Sw = np.sqrt(0.5) * np.sign(S2w) * np.sqrt(1 - C2w)
    YC, YS = Ch * Cw + Sh * Sw, Sh * Cw - Ch * Sw
    CC = 0.5 * (1 + C2 * C2w + S2 * S2w) - (C * Cw + S * Sw) ** 2
    SS = 0.5 * (1 - C2 * C2w - S2 * S2w) - (S * Cw - C * Sw) ** 2
    p = (YC * YC / CC + YS * YS / SS) * 0.5 * (wsum if dy is not None else len(t))
    if normalization == "psd":
        return p
    if normalization == "lk_amplitude":
        return np.sqrt(p) * np.sqrt(4.0 / len(t))
    if normalization == "lk_psd":
        return p * lk_scale
    raise ValueError(normalization)


@pytest.mark.parametrize("fit_mean,center_data,use_dy,norm",
                         list(itertools.product((True, False), (True, False), (False, True), ("psd", "standard"))))
def test_closed_form_equals_normal_equations(fit_mean, center_data, use_dy, norm):
    t, y, dy = target()
    d = dy if use_dy else None
    got = O.ls_power_fast(t, y, d, F0, DF, M, normalization=norm, fit_mean=fit_mean, center_data=center_data)
    ref = O.ls_power_fastchi2(t, y, d, F0, DF, M, nterms=1, fit_mean=fit_mean, center_data=center_data, normalization=norm)
    band = (F0 + DF * np.arange(M)) * (t.max() - t.min()) >= 1.0
    assert band.sum() > M // 2 and np.all(np.isfinite(ref[band])) and np.all(np.isfinite(got[band]))
    gap = np.max(np.abs(got[band] - ref[band])) / np.max(np.abs(ref[band]))
    print("fit_mean %d center_data %d dy %d %s: gap %.2e of the maximum" % (fit_mean, center_data, use_dy, norm, gap))
    assert gap <= TOL


def test_options_change_the_result():
    """The 16 cases are not one case 16 times: uncentred flux near 1 without the mean term is a different periodogram."""
    t, y, dy = target()
    a = O.ls_power_fast(t, y, dy, F0, DF, M)
    b = O.ls_power_fast(t, y, dy, F0, DF, M, fit_mean=False)
    c = O.ls_power_fast(t, y, dy, F0, DF, M, fit_mean=False, center_data=False)
    assert np.array_equal(a, O.ls_power_fast(t, y, dy, F0, DF, M, center_data=False))     # fit_mean centres by itself
    assert np.nanmax(np.abs(a - b)) > 1e-6 * np.nanmax(a) and np.nanmax(np.abs(b - c)) > 1e-3 * np.nanmax(b)
    assert not np.array_equal(a, O.ls_power_fast(t, y, dy, F0, DF, M, oversampling=2), equal_nan=True)


@pytest.mark.parametrize("use_dy", (False, True))
@pytest.mark.parametrize("norm", ("psd", "lk_amplitude", "lk_psd"))
def test_default_arguments_keep_their_bits(use_dy, norm):
    t, y, dy = target()
    d = dy if use_dy else None
    for f0 in (0.0, F0):
        new = O.ls_power_fast(t + 0.37, y, d, f0, DF, M, normalization=norm, lk_scale=3.7)
        old = fast_before_options(t + 0.37, y, d, f0, DF, M, normalization=norm, lk_scale=3.7)
        assert np.array_equal(new, old, equal_nan=True)


def test_fastchi2_idx_selects_the_full_result():
    t, y, dy = target()
    idx = np.array([0, 1, 17, 999, 998, M - 1])
    for kw in (dict(nterms=2), dict(nterms=1, fit_mean=False, normalization="standard")):
        full = O.ls_power_fastchi2(t, y, dy, F0, DF, M, **kw)
        assert np.array_equal(O.ls_power_fastchi2(t, y, dy, F0, DF, M, idx=idx, **kw), full[idx], equal_nan=True)
