"""Inputs and a pure numpy / scipy reference for the SFF tests (tests/test_sff_cpu.py, tests/test_sff_gpu.py).

The reference restates lightkurve 2.x ``correctors/sffcorrector.py`` with ``scipy.interpolate.BSpline.design_matrix`` on the
clamped knot vector for both bases and ``oracle.np_oracle.regression_correct`` for the fit.  Nothing here imports the package
under test.  Windows are cut by index (the stated deviation from the reference's by-value ``np.in1d``).
"""
import functools

import numpy as np
from scipy.interpolate import BSpline

from oracle import np_oracle as O

CADENCE = 0.0204          # days
BINS, DEGREE, TIMESCALE = 5, 3, 1.5
LEVEL = 1000.0            # flux level of the synthetic targets [e-/s]


def make_target(seed, N, negative_slope=False, t0=2000.0):
    """One K2-like target: 12-cadence sawtooth roll + drift + noise in the centroids; flux = slow sine + an arclength-dependent
    term + 3e-4 noise + three +0.02 spikes."""
    rng = np.random.RandomState(seed)
    i = np.arange(N)
    time = t0 + CADENCE * i + 1e-5 * rng.rand(N)
    roll = (i % 12) / 12.0
    theta = 0.6
    col = 10.3 + roll * np.cos(theta) + 2e-4 * i + 1e-3 * rng.randn(N)
    row = 20.7 + (-1.0 if negative_slope else 1.0) * roll * np.sin(theta) + 1e-4 * i + 1e-3 * rng.randn(N)
    flux = 1.0 + 0.003 * np.sin(2 * np.pi * (time - t0) / 6.0) + 0.006 * (roll - 0.4) ** 2 + 3e-4 * rng.randn(N)
    spikes = rng.choice(np.arange(20, N - 20), 3, replace=False)
    flux[spikes] += 0.02
    err = 3e-4 * (1.0 + 0.1 * rng.rand(N))
    return dict(time=time, flux=LEVEL * flux, flux_err=LEVEL * err, col=col, row=row, spikes=np.sort(spikes))


def even_points(N, windows):
    """Cut indices of `windows` windows, each starting right after a roll ends."""
    if windows == 1:
        return np.zeros(0, dtype=np.int64)
    return np.asarray([12 * int(round(N * k / windows / 12.0)) + 1 for k in range(1, windows)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def batch():
    """The three ragged targets (N = 600, 571, 640: n_knots = 8, 7, 8, so two design widths), the second with a negative
    row / column slope, windows = 4 each; plus a fourth whose baseline is shorter than 4 timescales."""
    # (seeds whose reference residuals stay clear of the 5-sigma decision in every clip iteration: test_sff_cpu.py checks it)
    targets = [make_target(13, 600), make_target(14, 571, negative_slope=True), make_target(16, 640), make_target(14, 200)]
    wps = [even_points(len(t["time"]), 4) for t in targets[:3]] + [even_points(200, 2)]
    return targets, wps


def pack(targets, key):
    return np.concatenate([t[key] for t in targets])


def offsets(targets):
    return np.concatenate([[0], np.cumsum([len(t["time"]) for t in targets])]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the reference
def arclength(col, row):
    c = col - np.min(col)
    r = row - np.min(row)
    flip = np.polyfit(c, r, 1)[0] < 0
    if flip:
        c = np.max(c) - c
    return np.sqrt(c * c + r * r), bool(flip)


def clamped_basis(x, lo, hi, inner, degree):
    t = np.concatenate([[lo] * (degree + 1), np.asarray(inner, float), [hi] * (degree + 1)])
    return BSpline.design_matrix(np.asarray(x, float), t, degree).toarray()


def n_knots_of(time, timescale=TIMESCALE):
    return int((time[-1] - time[0]) / timescale)


def design(time, f, arc, window_points, bins=BINS, degree=DEGREE, timescale=TIMESCALE):
    """-> X (N, K), prior_mu, prior_sigma, time knots [lo, inner..., hi], window knots (W, bins + 1)."""
    N = len(time)
    nk = n_knots_of(time, timescale)
    inner_t = np.percentile(time, np.linspace(0, 100, nk - 4 + 2)[1:-1])
    kt = np.concatenate([[time.min()], inner_t, [time.max()]])
    blocks = [clamped_basis(time, kt[0], kt[-1], inner_t, 3)]
    mu = [np.asarray([np.mean(c) for c in np.array_split(f, nk)])]
    sg = [np.full(nk, 1000 * np.std(f) + 1e-6)]
    lo = np.append(0, window_points).astype(int)
    up = np.append(window_points, N).astype(int)
    kw = []
    for a, b in zip(lo, up):
        inner = np.percentile(arc[a:b], np.linspace(0, 100, bins + 1)[1:-1])
        x = np.full(N, -1.0)
        x[a:b] = arc[a:b]
        kw.append(np.concatenate([[x.min()], inner, [x.max()]]))
        blocks.append(clamped_basis(x, x.min(), x.max(), inner, degree))
        mu.append(np.zeros(bins + degree))
        sg.append(np.full(bins + degree, 10000 * np.std(f) + 1e-6))
    return np.hstack(blocks), np.concatenate(mu), np.concatenate(sg), kt, np.asarray(kw)


def correct(t, window_points, restore_trend=False, cadence_mask=None, bins=BINS, degree=DEGREE, timescale=TIMESCALE, sigma=5.0,
            niters=5):
    """SFFCorrector.correct of one target dict -> dict(arclength, flip, X, prior_mu, prior_sigma, flux, flux_err, spline, sff,
    outlier_mask, coefficients, f, e, n_knots)."""
    time, flux, err = t["time"], t["flux"], t["flux_err"]
    med = np.nanmedian(flux)
    f, e = flux / med, err / med
    raw_mean = flux.mean()
    arc, flip = arclength(t["col"], t["row"])
    X, mu, sg, kt, kw = design(time, f, arc, window_points, bins, degree, timescale)
    nk = len(kt) + 2
    res = O.regression_correct(X, f, e, cadence_mask=cadence_mask, prior_mu=mu, prior_sigma=sg, sigma=sigma, niters=niters)
    w = res["coefficients"]
    spline = X[:, :nk].dot(w[:nk])
    spline = spline - np.median(spline)
    sff = X[:, nk:].dot(w[nk:])
    sff = sff - np.median(sff)
    corrected = f - res["model"]
    if restore_trend:
        corrected = corrected + (spline - np.nanmedian(spline))
    return dict(arclength=arc, flip=flip, X=X, prior_mu=mu, prior_sigma=sg, knots_time=kt, knots_win=kw, flux=corrected * raw_mean,
                flux_err=e * raw_mean, spline=spline, sff=sff, outlier_mask=res["outlier_mask"], coefficients=w, f=f, e=e,
                n_knots=nk)


@functools.lru_cache(maxsize=None)
def reference(index, restore_trend=False, masked=False, windows=4):
    """The reference result of target `index` of batch() (computed once and shared; treat as read-only)."""
    targets, wps = batch()
    t = targets[index]
    wp = wps[index] if windows == 4 else even_points(len(t["time"]), windows)
    return correct(t, wp, restore_trend=restore_trend, cadence_mask=cadence_mask(index) if masked else None)


def cadence_mask(index):
    """The cadence mask of the masked case: a stretch of 25 cadences and every 17th cadence left out of the fit."""
    targets, _ = batch()
    N = len(targets[index]["time"])
    m = np.ones(N, dtype=bool)
    m[100:125] = False
    m[::17] = False
    return m


def clip_margins(X, f, e, mu, sg, cadence_mask=None, sigma=5.0, niters=5):
    """|r - cen| / std of every residual against the final bounds of every clip iteration of the reference fit -> list of
    arrays (one per regression iteration): how far each residual is from the sigma = 5 decision."""
    n = len(f)
    cm = np.ones(n, bool) if cadence_mask is None else np.asarray(cadence_mask, bool)
    outl = np.zeros(n, bool)
    out = []
    for _ in range(niters):
        m = cm & ~outl
        Xm = X[m]
        A = Xm.T.dot(Xm / e[m, None] ** 2) + np.diag(1.0 / sg ** 2)
        b = Xm.T.dot(f[m] / e[m] ** 2) + mu / sg ** 2
        r = f - X.dot(np.linalg.solve(A, b))
        d = r.copy()
        for _ in range(5):
            cen, std = np.median(d), np.std(d)
            keep = np.abs(d - cen) <= sigma * std
            if keep.all():
                break
            d = d[keep]
        out.append(np.abs(r - cen) / std)
        outl |= O.sigma_clip_mask(r, sigma)
    return out
