"""Synthetic fields and the numpy restatement of the device noise generator, shared by test_overfit_cpu.py and
test_overfit_gpu.py (no test in here).

A field: B targets on shared times ``t = 1000 + 0.02 arange(N)``, flux ``1000 (1 + S a_b + 1e-3 noise)`` with three smooth
systematics S, errors ``1000 * 1e-3``.  Corrected variants of a field: ``a`` the original itself (metric exactly 1), ``b`` a
least-squares fit of [S | 1] removed with a de-medianed model (a good correction), ``c0.5`` ... ``c4`` variant b plus injected
white noise at 0.5, 1, 2 and 4 times the uncertainty (over-fitted corrections: the metric falls to about 0.07)."""
import functools

import numpy as np

VARIANTS = ("a", "b", "c0.5", "c1", "c2", "c4")
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ Philox4x32-10 / Box-Muller
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011; Random123) on arrays of 32-bit words held in uint64 -> four uint64 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def normals(n, k, target, seed=0, stream_id=0):
    """The n standard normals of (target, sample k): counter (i, k, target, stream_id) for the pair of cadences (2i, 2i + 1),
    key (seed & 0xffffffff, seed >> 32); Box-Muller on u1 in (0, 1], u2 in [0, 1)."""
    i = np.arange((n + 1) // 2, dtype=np.uint64)
    x0, x1, x2, x3 = philox4x32_10(i, k, target, stream_id, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u1 = (((x0 >> np.uint64(5)) << np.uint64(26)) + (x1 >> np.uint64(6)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (((x2 >> np.uint64(5)) << np.uint64(26)) + (x3 >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586 * u2
    out = np.empty(2 * len(i))
    out[0::2] = r * np.cos(ang)
    out[1::2] = r * np.sin(ang)
    return out[:n]


class RandnFromMirror(object):
    """Stands in for ``numpy.random.randn`` under a loop ``for target in targets: metric(..., n_samples)``: call number c
    returns the normals of (target first_target + c // n_samples, sample c % n_samples), in the shape asked for."""

    def __init__(self, n_samples, seed=0, first_target=0, stream_id=0):
        self.n_samples, self.seed, self.first_target, self.stream_id, self.calls = n_samples, seed, first_target, stream_id, 0

    def __call__(self, *shape):
        b, k = divmod(self.calls, self.n_samples)
        self.calls += 1
        return normals(int(np.prod(shape)), k, self.first_target + b, self.seed, self.stream_id).reshape(shape)


# ------------------------------------------------------------------------------------------------ fields
def systematics(N):
    x = np.linspace(-1.0, 1.0, N)
    return np.column_stack([x, np.sin(2.3 * x + 0.4), np.cos(5.1 * x) * x])


@functools.lru_cache(maxsize=None)
def field(N, B=5, seed=11):
    """-> dict(t (N,), S (N, 3), y (B, N), err (B, N), variants {name: corrected (B, N)}); cached: read-only arrays."""
    rng = np.random.default_rng(seed + 1000 * N)
    t = 1000.0 + 0.02 * np.arange(N)
    S = systematics(N)
    a = rng.normal(0, 0.01, (B, 3))
    y = 1000.0 * (1.0 + a @ S.T + 1e-3 * rng.normal(0, 1, (B, N)))
    err = np.full((B, N), 1000.0 * 1e-3)
    X = np.column_stack([S, np.ones(N)])
    model = (X @ np.linalg.lstsq(X, y.T, rcond=None)[0]).T
    fit = y - (model - np.median(model, axis=1)[:, None])
    variants = {"a": y.copy(), "b": fit}
    for s in (0.5, 1.0, 2.0, 4.0):
        variants["c%g" % s] = fit + s * err * rng.normal(0, 1, (B, N))
    for arr in [t, S, y, err] + list(variants.values()):
        arr.setflags(write=False)
    return dict(t=t, S=S, y=y, err=err, variants=variants)


def masks(N):
    """Two cadence masks of a field: one leaves an odd count of kept cadences, one an even count."""
    cm = np.ones(N, dtype=bool)
    cm[[1, N // 2]] = False
    other = cm.copy()
    other[N - 2] = False
    return (cm, other) if cm.sum() % 2 else (other, cm)


def default_grid(t):
    """The grid ``LombScarglePeriodogram.from_lightcurve`` builds (amplitude normalisation, oversample factor 5) [1/d]."""
    fs = (1.0 / (t[-1] - t[0])) / 5.0
    return np.arange(fs, 0.5 * (1.0 / np.median(np.diff(t))), fs)


# ------------------------------------------------------------------------------------------------ the closed form
def closed_form(ls, t, y0, y1, e1, n_samples, seed=0, first_target=0, stream_id=0, cm=None, frequency=None):
    """What overfit.hip computes, in numpy, with ``ls(t, rows, frequency) -> power[len(rows), M]`` as the periodogram and the
    mirror's normals as the noise -> (metric[B], margin[B]): margin = min |change| / max(P0, P1), how far the nearest entry of
    ``change`` is from rounding across zero (inf where the two spectra are the same bits)."""
    y0, y1, e1 = (np.asarray(v, dtype=np.float64) for v in (y0, y1, e1))
    B, N = y0.shape
    cm = np.ones(N, dtype=bool) if cm is None else np.asarray(cm, dtype=bool)
    tk = np.asarray(t, dtype=np.float64)[cm]
    n = len(tk)
    frequency = default_grid(tk) if frequency is None else np.asarray(frequency, dtype=np.float64)
    med1 = np.median(y1[:, cm], axis=1)[:, None]
    z0 = y0[:, cm] / np.median(y0[:, cm], axis=1)[:, None] - 1.0
    z1 = y1[:, cm] / med1 - 1.0
    mean_unc = np.nanmean(e1[:, cm] / med1, axis=1)
    P0, P1 = ls(tk, z0, frequency), ls(tk, z1, frequency)
    g = np.array([[normals(n, k, first_target + b, seed, stream_id) * mean_unc[b] for b in range(B)] for k in range(n_samples)])
    Pn = ls(tk, g.reshape(n_samples * B, n), frequency).reshape(n_samples, B, -1)
    metric, margin = np.empty(B), np.empty(B)
    with np.errstate(all="ignore"):
        for b in range(B):
            change = P1[b] - P0[b]
            change = change[~np.isnan(change)]
            margin[b] = np.inf if np.array_equal(P0[b], P1[b], equal_nan=True) else \
                np.min(np.abs(change)) / max(np.nanmax(P0[b]), np.nanmax(P1[b]))
            up = change > 0
            n_up, s = int(up.sum()), float(np.sum(change[up]))
            acc = 0.0
            for k in range(n_samples):
                if n_up == 0:
                    per = 0.0
                else:
                    den = n_up * np.nanmean(Pn[k, b])
                    per = np.inf if den == 0 else s / den
                acc += per
            mean = acc / n_samples
            metric[b] = 2.0 / (1.0 + np.exp(mean if np.isnan(mean) else max(mean, 0.0)))
    return metric, margin
