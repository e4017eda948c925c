"""Inputs and numpy restatements shared by test_select_cpu.py and test_select_gpu.py (no test in here).

  * ``sigma_clip_mask_asym``: astropy.stats.sigma_clip(y, sigma, sigma_lower, sigma_upper, maxiters, cenfunc=median,
    stdfunc=std).mask; ``oracle.np_oracle.sigma_clip_mask`` is its symmetric form.
  * ``cdpp_tail``: the tail of ``LightCurve.estimate_cdpp`` (reference lightcurve.py:1764-1833, utils.py:374-386).
  * ``ragged_batch``: the one ragged batch of the mask / select / CDPP tests: every wave and workgroup boundary of the kernels
    (64 lanes, 512- and 1024-thread workgroups), empty rows in the middle and at the end, an all-NaN row, a constant row, a
    row with +inf, rows with NaN flux; white noise of 3e-4 around 1 with about 1 % outliers, +0.01 up and -0.004 down, so
    asymmetric bounds select differently from symmetric ones.
  * ``bls_field`` / ``bls_search_oracle``: four light curves with two injected box transits and the planet-by-planet search
    on the CPU BLS oracle.
"""
import functools

import numpy as np

LENGTHS = (1023, 13, 64, 0, 1, 2, 63, 65, 1024, 1025, 2049, 4500)      # + the three special rows and a last empty one
PARAMS = (dict(sigma=5.0), dict(sigma_lower=20.0, sigma_upper=3.0), dict(sigma=3.0, maxiters=None), dict(sigma=4.0, maxiters=1))
DURATIONS = (1, 13, 64, 200)
SEED = 20240911
GUARD = 1e-9


def sigma_clip_mask_asym(y, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5, rounds=None):
    """The mask of astropy's sigma_clip with median / std (True = clipped or not finite).  ``rounds``: a list that receives
    (lo, hi, std) of every round."""
    lower = sigma if sigma_lower is None else sigma_lower
    upper = sigma if sigma_upper is None else sigma_upper
    r = np.asarray(y, dtype=np.float64)
    d = r[np.isfinite(r)]
    lo, hi = -np.inf, np.inf
    changed, it = True, 0
    while changed and d.size and (maxiters is None or it < maxiters):
        it += 1
        cen, std = np.median(d), np.std(d)
        lo, hi = cen - std * lower, cen + std * upper
        if rounds is not None:
            rounds.append((lo, hi, std))
        kept = d[(d >= lo) & (d <= hi)]
        changed = kept.size != d.size
        d = kept
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(r) | (r < lo) | (r > hi)


def clear_of_bounds(y, **params):
    """True if in every round of the restatement no finite value of the row lies within GUARD * std of lo or hi: then an
    ulp in the order of the std sum cannot move a cadence across a bound.  A round with std == 0 (constant values) is
    exempt: both bounds equal the value and equality keeps it."""
    rounds = []
    sigma_clip_mask_asym(y, rounds=rounds, **params)
    fin = np.asarray(y, dtype=np.float64)
    fin = fin[np.isfinite(fin)]
    for lo, hi, std in rounds:
        if std == 0:
            continue
        if np.any(np.abs(fin - lo) <= GUARD * std) or np.any(np.abs(fin - hi) <= GUARD * std):
            return False
    return True


def running_mean(data, window_size):
    if window_size > len(data):
        window_size = len(data)
    cumsum = np.cumsum(np.insert(data, 0, 0))
    return (cumsum[window_size:] - cumsum[:-window_size]) / float(window_size)


def cdpp_tail(flat, outlier, transit_duration):
    kept = np.asarray(flat, dtype=np.float64)
    if outlier is not None:
        kept = kept[~np.asarray(outlier, dtype=bool)]
    if kept.size == 0:
        return np.nan
    with np.errstate(invalid="ignore"):
        ppm = kept / np.nanmedian(kept) * 1e6
        return float(np.std(running_mean(ppm, transit_duration)))


def _noisy(rng, n):
    f = 1.0 + 3e-4 * rng.standard_normal(n)
    hit = rng.random(n) < 0.01
    up = rng.random(n) < 0.5
    f[hit & up] += 0.01
    f[hit & ~up] -= 0.004
    return f


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """-> dict(time, flux, flux_err, quality, n_off, rows): host arrays in batch layout; ``rows``: what each row is."""
    rng = np.random.default_rng(SEED)
    flux, rows = [], []
    for n in LENGTHS:
        f = _noisy(rng, n)
        kind = "noise"
        if n in (65, 2049, 4500):           # NaN flux in a few cadences
            f[rng.choice(n, size=max(1, n // 200), replace=False)] = np.nan
            kind = "noise+nan"
        if n == 1025:
            f[517] = np.inf
            kind = "noise+inf"
        flux.append(f), rows.append(kind)
    flux.append(np.full(70, np.nan)), rows.append("all-nan")
    flux.append(np.full(130, 1.0003)), rows.append("constant")
    flux.append(_noisy(rng, 300)), rows.append("noise")
    flux.append(np.zeros(0)), rows.append("noise")
    n_off = np.zeros(len(flux) + 1, dtype=np.int64)
    n_off[1:] = np.cumsum([len(f) for f in flux])
    ntot = int(n_off[-1])
    time = np.concatenate([1000.0 + 0.02 * np.arange(len(f)) for f in flux])
    return dict(time=time, flux=np.concatenate(flux), flux_err=2e-4 + 1e-5 * rng.random(ntot),
                quality=rng.integers(0, 1 << 20, ntot).astype(np.int32), n_off=n_off, rows=tuple(rows))


def row_slices(n_off):
    return [slice(int(n_off[b]), int(n_off[b + 1])) for b in range(len(n_off) - 1)]


def restated_mask(flux, n_off, **params):
    return np.concatenate([sigma_clip_mask_asym(flux[s], **params) for s in row_slices(n_off)] + [np.zeros(0, dtype=bool)])


# ------------------------------------------------------------------------------------------------ two-planet search
BLS_PERIODS = (2.1, 3.7)
BLS_DEPTHS = (4e-3, 2.5e-3)
BLS_DURATION = 0.15
BLS_GRID = np.linspace(1.0, 5.0, 401)
BLS_DURATIONS = np.array([0.1, 0.15, 0.2])


@functools.lru_cache(maxsize=None)
def bls_field():
    """B = 4 light curves of ~1500 cadences at 30-minute cadence with the two box transits of BLS_PERIODS -> dict(time, flux,
    flux_err, n_off)."""
    rng = np.random.default_rng(SEED + 1)
    ts, fs = [], []
    for b in range(4):
        n = 1500 - 7 * b
        t = 2000.0 + (30.0 / 1440.0) * np.arange(n) + rng.uniform(-2e-4, 2e-4, n)
        f = 1.0 + 3e-4 * rng.standard_normal(n)
        for per, depth in zip(BLS_PERIODS, BLS_DEPTHS):
            tt = t[0] + rng.uniform(0.3, per - 0.3)
            f[np.abs((t - tt + 0.5 * per) % per - 0.5 * per) < 0.5 * BLS_DURATION] -= depth
        ts.append(t), fs.append(f)
    n_off = np.zeros(5, dtype=np.int64)
    n_off[1:] = np.cumsum([len(t) for t in ts])
    time, flux = np.concatenate(ts), np.concatenate(fs)
    return dict(time=time, flux=flux, flux_err=np.full(time.size, 3e-4), n_off=n_off)


def bls_search_oracle(time, flux, flux_err, n_signals=2):
    """The planet-by-planet loop for ONE light curve on the CPU BLS oracle -> list of (period, duration, transit_time)."""
    from oracle import np_oracle as O
    found = []
    for _ in range(n_signals):
        tt, yy, ivar, t_ref = O.lk_bls_inputs(time, flux, flux_err)
        res = O.bls(tt, yy, ivar, BLS_GRID, BLS_DURATIONS)
        a = int(np.nanargmax(res[0]))
        box = (float(BLS_GRID[a]), float(res[3][a]), float(res[4][a] + t_ref + time[0]))
        found.append(box)
        keep = ~O.transit_mask(time, box[0], box[1], box[2])
        time, flux, flux_err = time[keep], flux[keep], flux_err[keep]
    return found


def near_harmonic(found, injected, step):
    """found within one grid step of injected * k or injected / k, k = 1, 2, 3."""
    cands = [injected * k for k in (1, 2, 3)] + [injected / k for k in (2, 3)]
    return any(abs(found - c) <= step * 1.000001 for c in cands)
