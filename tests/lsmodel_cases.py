"""Inputs shared by tests/test_lsmodel_gpu.py: the ragged batches at whose sizes ``ls_model_kernel`` can go wrong, the input
condition that makes a difference from ``ls_model_host`` a bug, and the prewhitening light curves.  Everything is built once
per process (``functools.lru_cache``) and never modified."""
import functools

import numpy as np

COND_MAX = 1e4          # bound on cond(X^T W X) of every fitted target: the reference's own normal equations are then well posed


def _times(rng, n, t_start, cadence, gap_at=None, gap=0.0):
    """n sorted, jittered times from t_start; a gap of ``gap`` days in front of cadence ``gap_at``."""
    step = np.full(n, cadence)
    step[0] = 0.0
    if gap_at is not None:
        step[gap_at] += gap
    t = t_start + np.cumsum(step) + rng.uniform(-0.3, 0.3, n) * cadence
    assert np.all(np.diff(t) > 0)
    return t


def _signal(rng, t, f, amplitude=6e-3, noise=2e-4):
    """A normalised light curve with three harmonics of f (so that every nterms finds something to fit)."""
    x = 2 * np.pi * f * (t - t[0])
    y = 1 + amplitude * (np.sin(x + 0.3) + 0.4 * np.cos(2 * x + 1.1) + 0.2 * np.sin(3 * x - 0.7))
    return y + noise * rng.standard_normal(len(t))


@functools.lru_cache(maxsize=None)
def model_batches():
    """Two ragged batches (B <= 8 each), per target (time, flux, flux_err, frequency [1/d]):

    small  2 cadences (n < K at nterms 1 with fit_mean: status -1), 3 (exactly determined), 63 / 64 / 65 (the edges of a wave)
    large  512 / 513 (the edges of the workgroup), 700 with a two-day gap, 4100 with flux x 3e4 and one NaN in flux_err
           (weights fall back to ones for that target); 513 and 700 carry finite errors (weights 1 / flux_err^2 when asked)
    """
    rng = np.random.default_rng(20260412)
    small, large = [], []
    t = np.array([2100.0, 2100.26])                      # f dt = 0.26: the two phases a quarter turn apart
    small.append((t, np.array([1.0021, 0.9984]), np.full(2, 2e-4), 1.0))
    t = np.array([2200.0, 2200.31, 2200.57])             # phases 0, 0.31, 0.57 of a turn
    small.append((t, np.array([1.0031, 0.9978, 1.0009]), np.full(3, 2e-4), 1.0))
    for n in (63, 64, 65):
        t = _times(rng, n, 2300.0 + n, 0.02)
        small.append((t, _signal(rng, t, 2.4), np.full(n, 2e-4), 2.4))
    for n in (512, 513):
        t = _times(rng, n, 2400.0 + n, 0.02)
        e = rng.uniform(1.5e-4, 4e-4, n) if n == 513 else np.full(n, 2e-4)
        large.append((t, _signal(rng, t, 1.37 + 0.001 * n), e, 1.37 + 0.001 * n))
    t = _times(rng, 700, 2500.0, 0.02, gap_at=250, gap=2.0)
    large.append((t, _signal(rng, t, 0.83), rng.uniform(1.5e-4, 4e-4, 700), 0.83))
    t = _times(rng, 4100, 2600.0, 0.02)
    e = np.full(4100, 9.0)
    e[1234] = np.nan
    large.append((t, 3e4 * _signal(rng, t, 0.4127), e, 0.4127))
    return {"small": tuple(small), "large": tuple(large)}


def pack(targets):
    """(time, flux, flux_err, n_off, frequency[B]) of a list of targets."""
    n_off = np.concatenate([[0], np.cumsum([len(c[0]) for c in targets])]).astype(np.int64)
    return (np.concatenate([c[0] for c in targets]), np.concatenate([c[1] for c in targets]),
            np.concatenate([c[2] for c in targets]), n_off, np.array([c[3] for c in targets], dtype=np.float64))


def weights(flux_err, use_flux_err):
    """The dy ``ls_model_host`` gets for one target: None (unit weights) unless asked for and all finite."""
    return flux_err if (use_flux_err and np.all(np.isfinite(flux_err))) else None


def design(t, f, nterms, fit_mean):
    x = 2 * np.pi * f * (t - t[0])
    cols = [np.ones_like(x)] if fit_mean else []
    for m in range(1, nterms + 1):
        cols += [np.sin(m * x), np.cos(m * x)]
    return np.column_stack(cols)


def check_input_condition(t, dy, f, nterms, fit_mean):
    """The condition under which a difference between the kernel and ``ls_model_host`` is a bug, asserted on the reference's
    side: cond(X^T W X) < COND_MAX for every fitted target, and for every target long enough to allow both (more than eight
    cadences) at least two cycles over the baseline with the highest fitted harmonic below the Nyquist frequency of the median
    step.  (With three cadences the two cannot hold together: the median step is T / 2, so Nyquist is 1 / T while two cycles
    need f >= 2 / T; those targets are held to the conditioning bound alone.)"""
    X = design(t, f, nterms, fit_mean)
    w = np.ones(len(t)) if dy is None else dy ** -2.0
    assert np.linalg.cond(X.T.dot(X * w[:, None])) < COND_MAX, (len(t), nterms, fit_mean)
    if len(t) > 8:
        assert f * (t[-1] - t[0]) >= 2.0, (len(t), f)
        assert nterms * f < 0.5 / np.median(np.diff(t)), (len(t), nterms, f)


# ------------------------------------------------------------------------------------------------ prewhitening
PW_COUNTS = (700, 1100, 1800, 2500)
PW_AMPLITUDES = (8e-3, 4e-3, 2e-3)
PW_MIN_POWER = 1e-3          # between what two fits leave of the last target (a peak of 3.6e-4) and the weakest injected amplitude


@functools.lru_cache(maxsize=None)
def prewhiten_case():
    """Four targets of 700 .. 2500 jittered cadences; three carry three well-separated sinusoids (amplitudes 8e-3, 4e-3, 2e-3
    over 2e-4 of noise), the last one only the first two.  Returns (targets [(time, flux)], injected [B][<= 3] frequencies,
    the shared grid of <= 2000 frequencies)."""
    rng = np.random.default_rng(20260413)
    targets, injected = [], []
    for b, n in enumerate(PW_COUNTS):
        t = _times(rng, n, 2700.0 + 40 * b, 0.0229)
        fs = (3.137 + 0.21 * b, 7.411 - 0.17 * b, 11.873 + 0.13 * b)
        if b == len(PW_COUNTS) - 1:                      # two signals, a tenth of a grid step from a grid point each: what the
            fs = (3.7706, 6.8981)                        # fit at the grid point leaves of them stays far below PW_MIN_POWER
        y = 1 + 2e-4 * rng.standard_normal(n)
        for a, f, ph in zip(PW_AMPLITUDES, fs, (0.4, 1.9, 4.1)):
            y = y + a * np.sin(2 * np.pi * f * (t - t[0]) + ph)
        targets.append((t, y))
        injected.append(fs)
    grid = 0.5 + 0.0075 * np.arange(2000)                # 0.5 .. 15.49 1/d
    return tuple(targets), tuple(injected), grid
