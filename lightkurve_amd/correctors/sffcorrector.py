"""SFFCorrector (self-flat-fielding, the K2 roll-motion correction) over the device path
(reference: lightkurve 2.x src/lightkurve/correctors/sffcorrector.py; include/lkhip.h: lk_sff_correct_batch).

The arclength, the per-window percentile knots, the block-structured design matrix with its priors, the regression and the
component models all run in ``liblkhip.so``; what stays on the host is the CHOICE of the windows (``sff_window_points``,
optionally snapped to thruster firings found by ``sff_thruster_firings``), which needs nothing but the arclength.

Stated deviation: a cadence is "outside" a window BY INDEX (not in ``[lo_j, up_j)``).  The reference decides it by value
(``~np.in1d(ar, ar[a:b])``, a workaround of its own); the two differ only when an arclength outside the window is bit-equal to
one inside it.
"""
import numpy as np

from .. import _capi
from ..lightcurve import LightCurve

__all__ = ["SFFCorrector", "sff_correct_batch", "sff_window_points", "sff_thruster_firings"]


def sff_thruster_firings(arclength):
    """Cadences at which the arclength jumps back (a thruster firing ends a roll) -> ascending indices.

    Modelled on the reference's ``_get_thruster_firings``: ``d2 = gradient(gradient(arclength))``; a Gaussian is fitted by
    Levenberg-Marquardt (``scipy.optimize.leastsq``, residuals weighted by the square root of the density, start amplitude 100,
    mean 0, stddev 0.01) to the density histogram of ``d2`` on ``arange(-0.5, 0.5, 1e-4)``; a cadence is a firing if
    ``|d2| > 5 stddev`` (the robust width 1.4826 MAD of ``d2`` stands in for a fit that is not finite or more than ten times
    wider than it: a sparse histogram leaves the fit free to go wide); within each run of consecutive firings the one with the
    largest ``|gradient(arclength)|`` is kept (the first of equals).  Parity with astropy's ``LevMarLSQFitter``, which the reference uses, has NOT been checked: astropy is not
    installed where this was written.  The device path never depends on this helper: ``window_points`` can always be passed in.
    """
    from scipy.optimize import leastsq
    arc = np.asarray(arclength, dtype=np.float64)
    if arc.ndim != 1 or arc.size < 3:
        return np.zeros(0, dtype=np.int64)
    g1 = np.gradient(arc)
    d2 = np.gradient(g1)
    ok = np.isfinite(d2)
    edges = np.arange(-0.5, 0.5, 0.0001)
    dens, edges = np.histogram(d2[ok], edges, density=True)
    x = edges[1:] - np.median(np.diff(edges))
    wgt = np.sqrt(np.where(np.isfinite(dens), dens, 0.0))

    def resid(p):
        return wgt * (p[0] * np.exp(-0.5 * ((x - p[1]) / p[2]) ** 2) - np.nan_to_num(dens))

    with np.errstate(all="ignore"):
        p, _ = leastsq(resid, [100.0, 0.0, 0.01])
    stddev = abs(float(p[2]))
    robust = 1.4826 * float(np.median(np.abs(d2[ok] - np.median(d2[ok]))))
    if not np.isfinite(stddev) or stddev == 0.0 or abs(float(p[1])) > 0.5 or (robust > 0.0 and stddev > 10.0 * robust):
        # the fit did not settle on the core (a sparse histogram constrains it only where a bin is occupied): the robust width
        stddev = robust
    hit = ok & (np.abs(d2) > 5.0 * stddev)
    idx = np.flatnonzero(hit)
    if idx.size == 0:
        return idx.astype(np.int64)
    runs = np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1)
    return np.asarray([r[np.argmax(np.abs(g1[r]))] for r in runs], dtype=np.int64)


def sff_window_points(n, windows, arclength=None, breakindex=None, thrusters=None):
    """Cut indices of the SFF windows of a light curve of ``n`` cadences (reference ``_get_window_points``): evenly spaced
    points ``arange(a, b, n / windows)`` between the break indices, each snapped to the nearest thruster firing ``+ 1`` when
    firings are known (``thrusters``: indices, or found from ``arclength`` by ``sff_thruster_firings``), merged with the break
    indices by ``unique``; a first / last point closer than 0.4 x the median window length to an end is dropped, and so is
    any point outside ``(0, n)``.  ``windows == 1`` returns the break indices alone.  -> ascending int64 array."""
    n, windows = int(n), int(windows)
    if windows < 1:
        raise ValueError("windows must be >= 1")
    if breakindex is None:
        breaks = np.zeros(0, dtype=np.int64)
    else:
        breaks = np.unique(np.atleast_1d(np.asarray(breakindex, dtype=np.int64)))
        breaks = breaks[(breaks > 0) & (breaks < n)]
    if windows == 1:
        return breaks
    dt = n / windows
    lower, upper = np.append(0, breaks), np.append(breaks, n)
    pts = np.hstack([np.asarray(np.arange(a, b, dt), dtype=np.int64) for a, b in zip(lower, upper)])
    if thrusters is None and arclength is not None:
        thrusters = sff_thruster_firings(arclength)
    th = np.zeros(0, dtype=np.int64) if thrusters is None else np.asarray(thrusters, dtype=np.int64).reshape(-1)
    th = np.unique(np.hstack([th, breaks]))
    if th.size:
        pts = np.asarray([th[np.argmin(np.abs(th - p))] + 1 for p in pts if p not in breaks], dtype=np.int64)
    pts = np.unique(np.hstack([pts, breaks])).astype(np.int64)
    if pts.size > 1:
        med = np.median(np.diff(pts))
        if pts[0] < 0.4 * med:
            pts = pts[1:]
        if pts.size and pts[-1] > n - 0.4 * med:
            pts = pts[:-1]
    return pts[(pts > 0) & (pts < n)]


def _centroids(lcs, centroid_col, centroid_row):
    cols = [np.asarray(c, dtype=np.float64) for c in centroid_col]
    rows = [np.asarray(r, dtype=np.float64) for r in centroid_row]
    if len(cols) != len(lcs) or len(rows) != len(lcs):
        raise ValueError("one centroid_col and one centroid_row array per light curve")
    for lc, c, r in zip(lcs, cols, rows):
        if c.shape != (len(lc),) or r.shape != (len(lc),):
            raise ValueError("centroids must have one value per cadence")
    return cols, rows


def sff_correct_batch(lcs, centroid_col, centroid_row, windows=20, bins=5, timescale=1.5, breakindex=None, degree=3,
                      restore_trend=False, window_points=None, cadence_mask=None, sigma=5, niters=5, max_scratch_bytes=None,
                      device=0):
    """``SFFCorrector(lc).correct(...)`` for a list of host light curves in ONE library call.  ``centroid_col`` /
    ``centroid_row``: one array per light curve; ``window_points``: one list of cut indices per light curve, or None (then
    ``sff_window_points`` runs per target on the arclength the device computes); ``cadence_mask``: one bool array per light
    curve or None.  Returns (list of corrected LightCurve, dict with per-target ``status``, ``window_points``, and lists of
    ``arclength`` / ``spline`` / ``sff`` / ``outlier_mask`` / ``coefficients``).  A target whose status is not 0 (too short, a
    non-finite input) comes back as NaN."""
    lcs = list(lcs)
    cols, rows = _centroids(lcs, centroid_col, centroid_row)
    n_off = np.zeros(len(lcs) + 1, dtype=np.int64)
    n_off[1:] = np.cumsum([len(lc) for lc in lcs])

    def cat(arrs):
        return np.concatenate(arrs) if arrs else np.zeros(0)

    col, row = cat(cols), cat(rows)
    if window_points is None:
        arc, _ = _capi.sff_arclength_batch(col, row, n_off, device=device)
        window_points = [sff_window_points(len(lc), windows, arc[n_off[b]:n_off[b + 1]], breakindex) for b, lc in enumerate(lcs)]
    cm = None if cadence_mask is None else cat([np.asarray(m, dtype=bool) for m in cadence_mask])
    # a light curve without any finite error is fitted with unit weights (regressioncorrector.py:157-158) and keeps its NaN errors
    no_err = [not np.any(np.isfinite(lc.flux_err)) for lc in lcs]
    errs = [np.ones(len(lc)) if no_err[b] else lc.flux_err for b, lc in enumerate(lcs)]
    res = _capi.sff_correct_batch(cat([lc.time for lc in lcs]), cat([lc.flux for lc in lcs]), cat(errs),
                                  col, row, n_off, window_points, bins=bins, degree=degree, timescale=timescale,
                                  restore_trend=restore_trend, cadence_mask=cm, sigma=sigma, niters=niters,
                                  max_scratch_bytes=max_scratch_bytes, device=device)
    out = []
    for b, lc in enumerate(lcs):
        new = lc.copy()
        new.flux = res["flux"][n_off[b]:n_off[b + 1]].copy()
        new.flux_err = lc.flux_err.copy() if no_err[b] else res["flux_err"][n_off[b]:n_off[b + 1]].copy()
        out.append(new)
    info = dict(status=res["status"], window_points=[np.asarray(w, dtype=np.int64) for w in window_points],
                coefficients=res["coefficients"])
    for key in ("arclength", "spline", "sff", "outlier_mask"):
        info[key] = [res[key][n_off[b]:n_off[b + 1]] for b in range(len(lcs))]
    return out, info


class SFFCorrector(object):
    """``lightkurve.correctors.SFFCorrector`` for one light curve: ``correct`` mirrors the reference's signature and leaves the
    same attributes behind (``window_points``, ``arclength``, ``diagnostic_lightcurves['spline' | 'sff']``, ``outlier_mask``,
    ``corrected_lc``)."""

    def __init__(self, lc):
        if np.any(~np.isfinite(lc.time)) or np.any(~np.isfinite(lc.flux)):
            raise ValueError("Input light curve has NaNs in time or flux. "
                             "Please remove NaNs before correction (e.g. using `lc = lc.remove_nans()`).")
        self.lc = lc
        self.raw_lc = lc
        self.window_points = None
        self.arclength = None
        self.outlier_mask = None
        self.coefficients = None
        self.corrected_lc = None
        self.diagnostic_lightcurves = None

    def __repr__(self):
        return "SFFCorrector (ID: {})".format(self.lc.targetid)

    def correct(self, centroid_col, centroid_row, windows=20, bins=5, timescale=1.5, breakindex=None, degree=3,
                restore_trend=False, window_points=None, cadence_mask=None, sigma=5, niters=5, device=0, **kwargs):
        """Fit the long-term spline and the per-window arclength splines together and remove the arclength part (and the
        long-term part too unless ``restore_trend``).  ``window_points`` overrides the automatic choice; ``**kwargs`` is
        accepted for the reference's signature and must be empty."""
        if kwargs:
            raise TypeError("unexpected keyword argument(s): %s" % sorted(kwargs))
        out, info = sff_correct_batch([self.lc], [centroid_col], [centroid_row], windows=windows, bins=bins, timescale=timescale,
                                      breakindex=breakindex, degree=degree, restore_trend=restore_trend,
                                      window_points=None if window_points is None else [window_points],
                                      cadence_mask=None if cadence_mask is None else [cadence_mask], sigma=sigma, niters=niters,
                                      device=device)
        status = int(info["status"][0])
        if status != 0:
            raise ValueError("SFFCorrector cannot correct this light curve: %s" % _capi.SFF_STATUS.get(status, status))
        self.centroid_col, self.centroid_row = np.asarray(centroid_col, float), np.asarray(centroid_row, float)
        self.windows, self.bins, self.timescale, self.breakindex = windows, bins, timescale, breakindex
        self.window_points = info["window_points"][0]
        self.arclength = info["arclength"][0]
        self.outlier_mask = info["outlier_mask"][0]
        self.cadence_mask = np.ones(len(self.lc), bool) if cadence_mask is None else np.asarray(cadence_mask, bool)
        self.coefficients = info["coefficients"][0]
        zeros = np.zeros(len(self.lc))
        self.diagnostic_lightcurves = {
            name: LightCurve(time=self.lc.time, flux=info[name][0], flux_err=zeros, label=name) for name in ("spline", "sff")}
        self.corrected_lc = out[0]
        return self.corrected_lc
