"""Over-fitting goodness metric on the GPU.

Reference: src/lightkurve/correctors/metrics.py:24-138 ``overfit_metric_lombscargle`` — per sample three default
(``ls_method="fast"``) Lomb-Scargle periodograms: the original light curve, the corrected one on the same grid, and a
white-noise light curve at the level of the corrected uncertainties; the metric compares the power the correction ADDED
with the noise power.  The first two periodograms do not depend on the sample, so they are computed once; the
``n_samples`` noise periodograms are one batched launch (``lombscargle_batch``).  The noise is drawn from the global
``np.random`` stream in the reference's order, so with the same seed the metric reproduces the reference's value.
"""
import numpy as np

from ..batch import lombscargle_batch
from ..lightcurve import LightCurve

__all__ = ["overfit_metric_lombscargle", "overfit_metric_lombscargle_batch", "underfit_metric_neighbors",
           "underfit_metric_batch", "nearest_neighbors", "overfit_metric_batch", "underfit_metric_ragged_batch",
           "overfit_metric_ragged_batch"]


def _prepared(lc):
    lc = lc.copy().remove_nans().normalize()
    return lc - 1.0


def overfit_metric_lombscargle(original_lc, corrected_lc, n_samples=10, device=0):
    """A float in [0, 1]: 0 = the correction injected broadband noise far above the uncertainties, 1 = none."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # zero-centred / zero-median light curves are expected here
        orig_lc = _prepared(original_lc)
        corrected_lc = _prepared(corrected_lc)
    if len(corrected_lc) == 0:
        return 1.0
    pg_orig = orig_lc.to_periodogram(device=device)
    pg_corr = corrected_lc.to_periodogram(frequency=pg_orig.frequency, device=device)
    n = len(orig_lc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mean_unc = np.nanmean(corrected_lc.flux_err)
    noise = [LightCurve(time=orig_lc.time, flux=(np.random.randn(n, 1) * mean_unc).T[0], flux_err=np.zeros(n))
             for _ in range(int(n_samples))]
    # a light curve's default grid depends on its times only: the noise curves share pg_orig's grid
    noise_power = lombscargle_batch(noise, pg_orig.frequency, device=device) if noise else np.zeros((0, 1))
    change = np.asarray(pg_corr.power) - np.asarray(pg_orig.power)
    change = change[~np.isnan(change)]
    n_up = int(np.count_nonzero(change > 0.0))
    per_iter = []
    for k in range(int(n_samples)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mean_noise_power = np.nanmean(noise_power[k])
        if n_up == 0:
            per_iter.append(0.0)
        else:
            den = n_up * mean_noise_power
            per_iter.append(np.inf if den == 0 else np.sum(change[change > 0.0]) / den)
    metric = np.mean(per_iter)
    with np.errstate(over="ignore"):
        return float(2.0 / (1.0 + np.exp(np.max([metric, 0.0]))))


def overfit_metric_batch(time, flux, flux_corrected, flux_err_corrected, frequency=None, n_samples=10, cadence_mask=None, seed=0,
                         first_target=0, stream_id=0, device=0, max_scratch_bytes=None):
    """``overfit_metric_lombscargle`` for every row of host arrays in ONE GPU call (``lk_overfit_metric_batch``): ``flux`` (the
    originals), ``flux_corrected``, ``flux_err_corrected`` (B, N; NaN-free flux) at ``time`` ((N,) shared by the targets, or
    (B, N)); ``cadence_mask`` bool (N,), True = used (the reference's ``lc[cadence_mask]``); ``frequency`` [1/d]: a regular
    grid, or None = the grid ``LombScarglePeriodogram.from_lightcurve`` builds for target 0's kept cadences.  The white noise
    does not come from ``numpy.random`` but from a counter-based generator on the device (Philox4x32-10 keyed by ``seed``,
    counter (cadence pair, sample, ``first_target`` + row, ``stream_id``): include/lkhip.h), so a target's value does not depend
    on the batch around it.  Returns metric[B].  A resident batch has the same call as
    ``DeviceLightCurveBatch.over_fitting_metric``: the same kernels, the same bits."""
    from .. import _capi
    return _capi.overfit_metric_batch(time, flux, flux_corrected, flux_err_corrected, frequency=frequency, n_samples=n_samples,
                                      cadence_mask=cadence_mask, seed=seed, first_target=first_target, stream_id=stream_id,
                                      device=device, max_scratch_bytes=max_scratch_bytes)


def overfit_metric_lombscargle_batch(original_lc, corrected_lcs, n_samples=1, device=0):
    """``overfit_metric_lombscargle(original_lc, c)`` for every corrected light curve ``c`` of a list that shares the
    cadences of ``original_lc`` (e.g. one correction per ridge penalty): the periodogram of the original is computed once,
    the len(corrected_lcs) corrected periodograms and all the noise periodograms are ONE batched GPU call each.  The noise
    draws follow the loop order of calling the scalar function once per light curve, so the values are the same as
    that loop's under the same seed."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        orig_lc = _prepared(original_lc)
        cors = [_prepared(c) for c in corrected_lcs]
    if not cors:
        return np.zeros(0)
    if any(len(c) != len(orig_lc) for c in cors):
        raise ValueError("every corrected light curve must share the cadences of the original")
    pg_orig = orig_lc.to_periodogram(device=device)
    freq = pg_orig.frequency
    n = len(orig_lc)
    corr_power = lombscargle_batch(cors, freq, device=device)
    noise, mean_unc = [], []
    for c in cors:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mu = np.nanmean(c.flux_err)
        mean_unc.append(mu)
        for _ in range(int(n_samples)):
            noise.append(LightCurve(time=orig_lc.time, flux=(np.random.randn(n, 1) * mu).T[0], flux_err=np.zeros(n)))
    noise_power = lombscargle_batch(noise, freq, device=device) if noise else np.zeros((0, len(freq)))
    out = np.empty(len(cors))
    for a in range(len(cors)):
        change = corr_power[a] - np.asarray(pg_orig.power)
        change = change[~np.isnan(change)]
        n_up = int(np.count_nonzero(change > 0.0))
        per_iter = []
        for k in range(int(n_samples)):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                mnp = np.nanmean(noise_power[a * int(n_samples) + k])
            if n_up == 0:
                per_iter.append(0.0)
            else:
                den = n_up * mnp
                per_iter.append(np.inf if den == 0 else np.sum(change[change > 0.0]) / den)
        metric = np.mean(per_iter) if per_iter else 0.0
        with np.errstate(over="ignore"):
            out[a] = 2.0 / (1.0 + np.exp(np.max([metric, 0.0])))
    return out


def underfit_metric_neighbors(corrected_lc, neighbor_flux):
    """Residual-correlation goodness (reference metrics.py:141-257) given the neighbours' flux on the cadences of
    ``corrected_lc`` (n_cadences x n_neighbours; the reference downloads and aligns them from MAST, :274-412 — control
    plane).  Pearson correlation of the normalised, median-subtracted target with each neighbour, the mean of the cubed
    absolute correlations scaled so that white-noise chance correlation maps to 0.95.  A (n_neighbours + 1)^2 correlation
    matrix of a few thousand cadences: host arithmetic, like the reference's."""
    import warnings
    nf = np.asarray(neighbor_flux, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        keep = ~np.isnan(corrected_lc.flux)
        lc = _prepared(corrected_lc)
    nf = nf[keep]
    flux_matrix = np.column_stack([nf, lc.flux])
    flux_matrix = flux_matrix[~np.any(np.isnan(flux_matrix), axis=1)]
    # _compute_correlation (metrics.py:451-475): columns scaled by their RMS (NOT mean-subtracted), then X^T X / n
    n_cad = flux_matrix.shape[0]
    rms = np.sqrt(np.sum(flux_matrix ** 2.0, axis=0) / n_cad)
    rms[rms == 0.0] = np.inf
    unit = flux_matrix / rms[None, :]
    corr = unit.T.dot(unit) / n_cad
    beta = [0.0007, 0.8083, -0.5023]
    wgn = beta[0] + beta[1] * (n_cad ** beta[2])
    bad_limit = 0.95
    scale = 1.0 / wgn * np.log((2.0 / bad_limit) - 1.0)
    corr = np.tril(corr, k=-1) + np.triu(corr, k=+1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = scale * np.nanmean(np.abs(corr) ** 3, axis=0)[-1]
    return float(2.0 / (1.0 + np.exp(c)))


def underfit_metric_batch(flux, neighbors, cadence_mask=None, device=0, return_correlations=False):
    """``underfit_metric_neighbors`` for every row of a host array ``flux`` (B, N; NaN-free) in ONE GPU call
    (``lk_underfit_neighbors_batch``), the neighbours of a target being other rows of ``flux``: ``neighbors`` int (B, M), row
    t = the indices of t's neighbours padded with -1 (``nearest_neighbors`` builds it from positions); ``cadence_mask`` bool
    (N,), shared by every target, True = used (the reference's ``lc[cadence_mask]``).  Returns metric[B], and with
    ``return_correlations`` also correlations[B, M] (NaN at padding).  A resident batch has the same call as
    ``DeviceLightCurveBatch.under_fitting_metric``: the same kernels, the same bits."""
    from .. import _capi
    r = _capi.underfit_neighbors_batch(flux, neighbors, cadence_mask=cadence_mask, device=device)
    return (r["metric"], r["correlations"]) if return_correlations else r["metric"]


def underfit_metric_ragged_batch(flux_list, cadenceno_list, grid, neighbors, cadence_mask_list=None, device=0,
                                 return_correlations=False, return_common=False):
    """``underfit_metric_neighbors`` for B host light curves that do NOT share all their cadences, in ONE GPU call
    (``lk_underfit_grid_neighbors_batch``): ``flux_list[b]`` (n_b,; NaN-free) at the integer cadence numbers
    ``cadenceno_list[b]`` (strictly increasing), ``grid`` the strictly increasing cadence numbers of the field (a cadence that is
    not on it is dropped, as ``CotrendingBasisVectors.align`` does); ``neighbors`` int (B, M) as in ``underfit_metric_batch``;
    ``cadence_mask_list[b]`` bool (n_b,), True = used.  As in the reference, a target is compared with its neighbours on the
    cadences that it and ALL of them have (``n_common``); fewer than two: NaN.  Returns metric[B], then correlations[B, M]
    (``return_correlations``) and n_common[B] (``return_common``).  A resident batch has the same call as
    ``DeviceLightCurveBatch.under_fitting_metric(cadenceno=)``: the same kernels, the same bits."""
    from .. import _capi
    grid = np.asarray(grid)
    if grid.ndim != 1 or grid.size < 1 or not np.issubdtype(grid.dtype, np.integer) or np.any(np.diff(grid) <= 0):
        raise ValueError("grid must be a 1-D array of strictly increasing integer cadence numbers")
    B = len(flux_list)
    if B < 1 or len(cadenceno_list) != B or (cadence_mask_list is not None and len(cadence_mask_list) != B):
        raise ValueError("flux_list, cadenceno_list (and cadence_mask_list) must hold one entry per light curve, at least one")
    flux, rows, masks, n_off = [], [], [], [0]
    for b in range(B):
        f = np.asarray(flux_list[b], dtype=np.float64)
        c = np.asarray(cadenceno_list[b])
        if f.ndim != 1 or c.shape != f.shape or not np.issubdtype(c.dtype, np.integer):
            raise ValueError("light curve %d: flux (n,) and integer cadenceno (n,) must match (got %s and %s)" % (b, f.shape, c.shape))
        if np.any(np.diff(c) <= 0):
            raise ValueError("light curve %d: its cadence numbers must be strictly increasing" % b)
        m = np.ones(f.size, dtype=bool) if cadence_mask_list is None else np.asarray(cadence_mask_list[b], dtype=bool)
        if m.shape != f.shape:
            raise ValueError("light curve %d: cadence_mask must have one entry per cadence (got %s)" % (b, m.shape))
        r = np.searchsorted(grid, c)
        on = (r < grid.size) & (grid[np.minimum(r, grid.size - 1)] == c)
        flux.append(f[on])
        rows.append(r[on])
        masks.append(m[on])
        n_off.append(n_off[-1] + int(on.sum()))
    res = _capi.underfit_grid_neighbors_batch(np.concatenate(flux), n_off, np.concatenate(rows).astype(np.int32), grid.size, neighbors,
                                              cadence_mask=None if cadence_mask_list is None else np.concatenate(masks),
                                              device=device)
    out = (res["metric"],)
    if return_correlations:
        out += (res["correlations"],)
    if return_common:
        out += (res["n_common"],)
    return out if len(out) > 1 else out[0]


def overfit_metric_ragged_batch(time_list, flux_list, flux_corrected_list, flux_err_corrected_list, frequency=None, n_samples=10,
                                cadence_mask_list=None, seed=0, first_target=0, stream_id=0, device=0, max_scratch_bytes=None):
    """``overfit_metric_batch`` for B host light curves of DIFFERENT lengths in ONE GPU call (``lk_overfit_metric_rows_batch``):
    per target ``time_list[b]``, ``flux_list[b]`` (the original), ``flux_corrected_list[b]``, ``flux_err_corrected_list[b]``
    (n_b,; NaN-free flux) and ``cadence_mask_list[b]`` bool (n_b,), True = used; ``frequency`` [1/d]: a regular grid shared by the
    targets, None = the default grid of target 0's kept times.  The noise of target b is that of the uniform call with
    ``first_target + b``.  Returns metric[B].  A resident batch has the same call as
    ``DeviceLightCurveBatch.over_fitting_metric``: the same kernels, the same bits."""
    from .. import _capi
    B = len(time_list)
    lists = (flux_list, flux_corrected_list, flux_err_corrected_list) + (() if cadence_mask_list is None else (cadence_mask_list,))
    if B < 1 or any(len(x) != B for x in lists):
        raise ValueError("every list must hold one entry per light curve, at least one")
    t = [np.asarray(a, dtype=np.float64).reshape(-1) for a in time_list]
    for b in range(B):
        for x in lists:
            if np.shape(x[b]) != t[b].shape:
                raise ValueError("light curve %d: every array must have its %d cadences (got shape %s)" % (b, t[b].size, np.shape(x[b])))
    n_off = np.concatenate([[0], np.cumsum([a.size for a in t])]).astype(np.int64)
    cat = lambda x: np.concatenate([np.asarray(a).reshape(-1) for a in x])
    return _capi.overfit_metric_rows_batch(cat(t), cat(flux_list), cat(flux_corrected_list), cat(flux_err_corrected_list), n_off,
                                           frequency=frequency, n_samples=n_samples,
                                           cadence_mask=None if cadence_mask_list is None else cat(cadence_mask_list), seed=seed,
                                           first_target=first_target, stream_id=stream_id, device=device,
                                           max_scratch_bytes=max_scratch_bytes)


def nearest_neighbors(x, y, n_neighbors=50, chunk=1024):
    """The ``min(n_neighbors, B - 1)`` nearest other targets of each of B targets at planar coordinates (``x``, ``y``) ->
    int32 (B, min(n_neighbors, B - 1)), nearest first, ties broken by index, the target itself never listed (the reference
    takes the nearest targets on the sky from a MAST search, metrics.py:274-412).  Targets are handled ``chunk`` at a time,
    so no B x B matrix exists."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError("x and y must have one entry per target each (got %d and %d)" % (x.size, y.size))
    B = x.size
    k = int(min(int(n_neighbors), B - 1))
    if k <= 0:
        return np.zeros((B, 0), dtype=np.int32)
    out = np.empty((B, k), dtype=np.int32)
    for a in range(0, B, int(chunk)):
        e = min(a + int(chunk), B)
        d2 = (x[a:e, None] - x[None, :]) ** 2 + (y[a:e, None] - y[None, :]) ** 2
        d2[np.arange(e - a), np.arange(a, e)] = np.inf          # never the target itself
        out[a:e] = np.argsort(d2, axis=1, kind="stable")[:, :k]   # stable: equal distances stay in index order
    return out
