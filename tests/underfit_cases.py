"""Synthetic fields and numpy references shared by test_underfit_cpu.py and test_underfit_gpu.py (no test in here).

A field: B targets of N cadences that share two systematic trends S with per-target amplitudes, plus white noise; a cadence
mask that drops about a tenth of the cadences; per target M neighbours drawn from the other targets.  The raw flux is
strongly correlated between targets (low under-fitting metric); with [S, 1] fitted out it is white (metric near 1)."""
import functools

import numpy as np

from lightkurve_amd import LightCurve
from lightkurve_amd.correctors.metrics import underfit_metric_neighbors

# (seed, B, N, M) -> kept cadences 902, 464, 1820, 115
CONFIGS = [(21, 37, 1003, 5), (22, 19, 517, 3), (23, 80, 2050, 70), (24, 9, 130, 8)]


def trends(N):
    t = np.linspace(0, 27, N)
    return t, np.column_stack([np.sin(2 * np.pi * t / 13.7), (t / 27 - 0.5) ** 2])


def permuted_neighbors(rng, B, M):
    """Row t: the first M entries of a permutation of the other targets."""
    nb = np.empty((B, M), dtype=np.int32)
    for t in range(B):
        others = np.delete(np.arange(B), t)
        nb[t] = rng.permutation(others)[:M]
    return nb


@functools.lru_cache(maxsize=None)
def field(seed, B, N, M):
    """-> dict(t, S, y (B, N), cm (N,) bool, neighbors (B, M) int32); cached: treat the arrays as read-only."""
    rng = np.random.default_rng(seed)
    t, S = trends(N)
    a = rng.normal(0, 0.01, (B, 2))
    y = 1000.0 * rng.uniform(0.5, 2, (B, 1)) * (1 + a @ S.T + 1e-3 * rng.normal(0, 1, (B, N)))
    cm = rng.random(N) > 0.1
    nb = permuted_neighbors(rng, B, M)
    for arr in (t, S, y, cm, nb):
        arr.setflags(write=False)
    return dict(t=t, S=S, y=y, cm=cm, neighbors=nb)


def detrended(y, S, cm):
    """y with the least-squares fit of [S, 1] on the kept cadences taken out (zero-centred, like cbv_correct's output)."""
    X = np.column_stack([S, np.ones(len(S))])
    w = np.linalg.lstsq(X[cm], y[:, cm].T, rcond=None)[0]
    return y - (X @ w).T


def rounding_bounds(n):
    """(correlation, metric) bounds on the difference between two correct float64 evaluations at n kept cadences.  A
    correlation is a ratio of n-term dot products: each evaluation carries at most about n 2^-53 of relative error in a dot
    (plus a few roundings), the value is at most 1 in magnitude, and two evaluations differ by at most twice that: 4 n 2^-53
    with room for the normalisation.  The metric 2 / (1 + exp(scale s / (m + 1))), s = sum of m cubes, has slope at most
    scale / (2 (m + 1)) in s, and s moves by at most 3 m times the correlation's error: 1.5 scale times the bound above."""
    c = 4.0 * n * 2.0 ** -53
    scale = np.log(2 / 0.95 - 1) / (0.0007 + 0.8083 * n ** (-0.5023))
    return c, 1.5 * scale * c


def mirror(y, neighbors, cm=None, t=None):
    """The repository's own ``underfit_metric_neighbors`` per target -> (metric[B], correlations[B, M]); the correlations are
    the last row of the mirror's correlation matrix (its arithmetic: columns over their RMS, X^T X / n), NaN at padding."""
    y = np.asarray(y, dtype=np.float64)
    B, N = y.shape
    cm = np.ones(N, dtype=bool) if cm is None else np.asarray(cm, dtype=bool)
    t = np.arange(N, dtype=np.float64) if t is None else t
    nb = np.asarray(neighbors).reshape(B, -1)
    with np.errstate(all="ignore"):
        z = y[:, cm] / np.median(y[:, cm], axis=1)[:, None] - 1.0
        metric = np.empty(B)
        corr = np.full(nb.shape, np.nan)
        n = int(cm.sum())
        for b in range(B):
            pos = np.nonzero(nb[b] >= 0)[0]
            cols = z[nb[b, pos]].T if len(pos) else np.zeros((n, 0))
            metric[b] = underfit_metric_neighbors(LightCurve(t[cm], y[b, cm]), cols)
            fm = np.column_stack([cols, z[b]])
            rms = np.sqrt(np.sum(fm ** 2.0, axis=0) / n)
            rms[rms == 0.0] = np.inf
            unit = fm / rms[None, :]
            corr[b, pos] = (unit.T.dot(unit) / n)[-1, :len(pos)]
    return metric, corr


def closed_form(y, neighbors, cm=None):
    """The formula the kernels implement, in numpy -> (metric[B], correlations[B, M])."""
    y = np.asarray(y, dtype=np.float64)
    B, N = y.shape
    cm = np.ones(N, dtype=bool) if cm is None else np.asarray(cm, dtype=bool)
    nb = np.asarray(neighbors).reshape(B, -1)
    n = int(cm.sum())
    with np.errstate(all="ignore"):
        z = y[:, cm] / np.median(y[:, cm], axis=1)[:, None] - 1.0
        g = np.einsum("bi,bi->b", z, z)
        wgn = 0.0007 + 0.8083 * n ** (-0.5023)
        scale = np.log(2 / 0.95 - 1) / wgn
        metric = np.empty(B)
        corr = np.full(nb.shape, np.nan)
        for b in range(B):
            s, m = 0.0, 0
            for p, j in enumerate(nb[b]):
                if j < 0:
                    continue
                c = 0.0 if (g[b] == 0 or g[j] == 0) else float(z[b] @ z[j]) / np.sqrt(g[b] * g[j])
                corr[b, p] = c
                s += abs(c) ** 3
                m += 1
            metric[b] = 2 / (1 + np.exp(scale * s / (m + 1)))
    return metric, corr
