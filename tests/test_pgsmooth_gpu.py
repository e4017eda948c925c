"""GPU parity: Periodogram.smooth / Periodogram.flatten through the C ABI vs the reference-generated
golden vectors (lightkurve `pg.smooth(method=...)`, `pg.flatten(return_trend=True)`) and the oracle restatement.

Tolerance (stated): 'logmedian' is selection (exact medians) + a short ordered sum, 'boxkernel' a short dot product in
the reference's order: max |gpu - ref| <= 1e-12 * max |ref|; NaN positions identical.
"""
import numpy as np
import pytest

from lightkurve_amd import _capi
from lightkurve_amd.periodogram import Periodogram, SNRPeriodogram, _box1d_kernel, _logmedian_windows
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-12


def relmax(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))


def same(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    if (~na).any():
        scale = np.max(np.abs(b[~nb]))
        assert np.max(np.abs(a[~na] - b[~nb])) <= TOL * scale


def test_golden_smooth_and_flatten(golden):
    g = golden("pg_smooth")
    pg = Periodogram(g["frequency"], g["power"], frequency_unit="uHz", power_unit="flux^2/uHz")
    for fw in (0.01, 0.05, 0.3):
        same(pg.smooth(method="logmedian", filter_width=fw).power, g["logmedian_%g" % fw])
    for fw in (3.0, 10.5, 40.0):
        same(pg.smooth(method="boxkernel", filter_width=fw).power, g["boxkernel_%g" % fw])
    snr, bkg = pg.flatten(return_trend=True)
    assert isinstance(snr, SNRPeriodogram)
    same(bkg.power, g["flatten_bkg"])
    same(snr.power, g["flatten_snr"])
    pgn = Periodogram(g["frequency"], g["power_nan"], frequency_unit="uHz")
    same(pgn.smooth(method="logmedian", filter_width=0.02).power, g["logmedian_nan"])
    same(pgn.smooth(method="boxkernel", filter_width=10.5).power, g["boxkernel_nan"])


def test_batch_vs_oracle_and_errors():
    rng = np.random.default_rng(5)
    M, B = 3001, 5
    f = 0.5 + 0.01 * np.arange(M)
    power = rng.chisquare(2, size=(B, M)) * (1.0 + 50.0 / f)
    power[1, 100:140] = np.nan          # a NaN run longer than the small kernel
    power[3, :] = np.nan                # all-NaN row
    tabs = _logmedian_windows(f, 0.03)
    out = _capi.pg_logmedian_batch(power, *tabs)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b in range(B):
            same(out[b], O.pg_smooth_logmedian(f, power[b], 0.03))
        for w in (1, 6, 31):
            out = _capi.pg_boxsmooth_batch(power, _box1d_kernel(w))
            for b in range(B):
                same(out[b], O.convolve_fill(power[b], O.box1d_kernel(w)))
    pg = Periodogram(1.0 / np.linspace(0.1, 5, 50)[::-1], np.ones(50))
    with pytest.raises(ValueError, match="evenly spaced"):
        pg.smooth(method="boxkernel", filter_width=0.1)
    with pytest.raises(ValueError, match="larger than 0"):
        Periodogram(f, power[0]).smooth(method="boxkernel", filter_width=0.0)
    with pytest.raises(ValueError):
        _capi.pg_boxsmooth_batch(power, np.ones(4))   # even tap count


def _value_class_rows(M, rng):
    """Rows of M samples from the value classes the radix select behind pg_window_median_kernel is otherwise never fed."""
    g = rng.standard_normal(M)
    i = np.arange(M)
    rows = {
        "negative": -rng.chisquare(2, M),
        "mixed_sign": g,
        "both_zeros": np.where(i % 3 == 0, 0.0, np.where(i % 3 == 1, -0.0, g)),
        "denormals": rng.integers(0, 64, M) * 5e-324,
        "two_valued": np.where(i % 2 == 0, 1.0, 2.0),            # an even window's two middle ranks are different values
        "ties": np.round(g, 1),
        "full_range": rng.uniform(-1.0, 1.0, M) * 1.7e308,       # the mean of the two middle ranks may overflow
        "some_plus_inf": np.where(i % 7 == 0, np.inf, g),
        "some_minus_inf": np.where(i % 5 == 0, -np.inf, g),
        "both_infs": np.where(i % 2 == 0, -np.inf, np.inf),      # even windows: the mean of -inf and +inf is NaN
        "mostly_inf": np.where(i % 4 != 0, np.inf, g),
        "with_nans": np.where(i % 6 == 0, np.nan, g),            # nanmedian: the count changes
    }
    return list(rows), np.array([rows[k] for k in rows])


def _median_of_kept(x):
    s = np.sort(x[~np.isnan(x)])
    c = s.size
    if c == 0:
        return np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        return s[(c - 1) // 2] if c & 1 else 0.5 * (s[c // 2 - 1] + s[c // 2])


def test_window_medians_are_exact_order_statistics_for_every_value_class():
    """pg_window_median_kernel's block_median (the 8-pass radix select on sortable keys) is otherwise only fed positive
    chi-square powers.  Hand-made window tables in which every frequency belongs to exactly ONE window make the output the
    window median itself, (0 + median / corr) / 1, so it is compared with `==` (value equality; NaN where the reference is NaN):
    windows of 1, 2, 255, 256 and 257 samples side by side, and one window that covers the whole row."""
    rng = np.random.default_rng(17)
    sizes = [1, 2, 255, 256, 257]
    M = sum(sizes)
    names, power = _value_class_rows(M, rng)
    hi = np.cumsum(sizes)
    lo = hi - sizes
    which = np.repeat(np.arange(len(sizes)), sizes)
    corr = (8.0 / 9.0) ** 3
    for wl, wh, k in ((lo, hi, which), (np.array([0]), np.array([M]), np.zeros(M, int))):
        out = _capi.pg_logmedian_batch(power, wl, wh, k, k, corr=corr)
        for b, name in enumerate(names):
            with np.errstate(invalid="ignore", over="ignore"):
                ref = np.array([_median_of_kept(power[b, l:h]) for l, h in zip(wl, wh)])[k] / corr
            ok = (out[b] == ref) | (np.isnan(out[b]) & np.isnan(ref))
            assert ok.all(), (name, len(wl), np.flatnonzero(~ok)[:5], out[b][~ok][:5], ref[~ok][:5])


def test_logmedian_over_value_classes_vs_oracle():
    """The same value classes through the front end's own window tables (overlapping log-frequency windows) against the
    oracle.  Finite rows: this file's same().  Rows that hold +-inf: same() scales by max |ref| and cannot take infinities, so
    the positions and signs of the non-finite outputs must be identical and same() covers the finite positions."""
    import warnings
    rng = np.random.default_rng(18)
    M = 3001
    f = 0.5 + 0.01 * np.arange(M)
    names, power = _value_class_rows(M, rng)
    tabs = _logmedian_windows(f, 0.03)
    out = _capi.pg_logmedian_batch(power, *tabs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b, name in enumerate(names):
            with np.errstate(all="ignore"):
                ref = O.pg_smooth_logmedian(f, power[b], 0.03)
            fin = np.isfinite(ref)
            assert np.array_equal(fin, np.isfinite(out[b])), name
            assert np.array_equal(np.isnan(ref), np.isnan(out[b])), name
            assert np.array_equal(np.sign(ref[~fin & ~np.isnan(ref)]), np.sign(out[b][~fin & ~np.isnan(ref)])), name
            if fin.any():
                same(out[b][fin], ref[fin])
