"""Ridge-prior CBV correction over the GPU regression path.

Reference: src/lightkurve/correctors/cbvcorrector.py:221-292 ``CBVCorrector.correct_gaussian_prior`` with
``_correct_initialization`` (:639-757) and ``_set_prior_width`` (:759-778): the design-matrix collection is
[selected cotrending basis vectors, optional extra design matrix, a constant column], every column gets the same
Gaussian prior width ``sigma = median(flux_err) / sqrt(|alpha|)`` (``alpha == 0`` -> no prior), and the fit is
``RegressionCorrector.correct``.  Reading CBV FITS files / MAST is the reference's control plane and stays there: the
basis vectors are handed in as an array interpolated to the light curve's cadences (what ``cbvs.to_designmatrix``
yields).

``correct`` (:397-500) is the goodness-metric optimisation: a bounded Brent search over the ridge penalty ``alpha`` of
``_goodness_metric_obj_fun`` (:781-854), each evaluation = one ridge fit (the regression kernels) + the over-fitting
metric (``correctors/metrics.py``: batched default Lomb-Scargle periodograms on the FFT path) and, if neighbour light
curves are supplied, the under-fitting metric.  ``goodness_scan`` evaluates the same objective for MANY alphas in two
GPU calls (one batched regression, one batched periodogram) — what a coarse pre-scan or a plot of the metrics against
alpha needs.  The search driver restates scipy.optimize.minimize_scalar(method='Bounded') (scipy
optimize/_optimize.py:_minimize_scalar_bounded), which is what the reference calls.
"""
import numpy as np

from .. import _capi
from .designmatrix import DesignMatrix, DesignMatrixCollection
from .metrics import overfit_metric_lombscargle, overfit_metric_lombscargle_batch, underfit_metric_neighbors
from .regressioncorrector import RegressionCorrector

__all__ = ["CBVCorrector", "minimize_scalar_bounded", "BoundedBrentBatch", "interpolate_cbvs", "pchip_slopes"]


def minimize_scalar_bounded(func, bounds, xatol=1e-5, maxiter=500):
    """scipy.optimize.minimize_scalar(func, method='Bounded', bounds=bounds, options={'maxiter': maxiter}) restated
    (Brent's fminbound: golden-section steps with parabolic interpolation; scipy optimize/_optimize.py
    ``_minimize_scalar_bounded``) so the optimisation needs no scipy in the product interpreter.  Given the same
    objective values it visits the same abscissae.  Returns dict(x, fun, nfev, status)."""
    x1, x2 = float(bounds[0]), float(bounds[1])
    if not (np.isfinite(x1) and np.isfinite(x2)):
        raise ValueError("Optimization bounds must be finite scalars.")
    if x1 > x2:
        raise ValueError("The lower bound exceeds the upper bound.")
    flag = 0
    sqrt_eps = np.sqrt(2.2e-16)
    golden_mean = 0.5 * (3.0 - np.sqrt(5.0))
    a, b = x1, x2
    fulc = a + golden_mean * (b - a)
    nfc, xf = fulc, fulc
    rat = e = 0.0
    x = xf
    fx = func(x)
    num = 1
    fu = np.inf
    ffulc = fnfc = fx
    xm = 0.5 * (a + b)
    tol1 = sqrt_eps * np.abs(xf) + xatol / 3.0
    tol2 = 2.0 * tol1
    while np.abs(xf - xm) > (tol2 - 0.5 * (b - a)):
        golden = 1
        if np.abs(e) > tol1:                      # try a parabolic step
            golden = 0
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = np.abs(q)
            r = e
            e = rat
            if (np.abs(p) < np.abs(0.5 * q * r)) and (p > q * (a - xf)) and (p < q * (b - xf)):
                rat = (p + 0.0) / q
                x = xf + rat
                if ((x - a) < tol2) or ((b - x) < tol2):
                    si = np.sign(xm - xf) + ((xm - xf) == 0)
                    rat = tol1 * si
            else:
                golden = 1
        if golden:
            e = a - xf if xf >= xm else b - xf
            rat = golden_mean * e
        si = np.sign(rat) + (rat == 0)
        x = xf + si * np.maximum(np.abs(rat), tol1)
        fu = func(x)
        num += 1
        if fu <= fx:
            if x >= xf:
                a = xf
            else:
                b = xf
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
            else:
                b = x
            if (fu <= fnfc) or (nfc == xf):
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
            elif (fu <= ffulc) or (fulc == xf) or (fulc == nfc):
                fulc, ffulc = x, fu
        xm = 0.5 * (a + b)
        tol1 = sqrt_eps * np.abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= maxiter:
            flag = 1
            break
    if np.isnan(xf) or np.isnan(fx) or np.isnan(fu):
        flag = 2
    return dict(x=float(xf), fun=float(fx), nfev=num, status=flag)


def _bounded_brent_steps(x1, x2, xatol, maxiter):
    """``minimize_scalar_bounded`` turned inside out: a generator that yields each abscissa where the function would call
    ``func`` and is sent the value; the same operations in the same order, statement for statement.  Its return value
    (``StopIteration.value``) is the function's dict."""
    flag = 0
    sqrt_eps = np.sqrt(2.2e-16)
    golden_mean = 0.5 * (3.0 - np.sqrt(5.0))
    a, b = x1, x2
    fulc = a + golden_mean * (b - a)
    nfc, xf = fulc, fulc
    rat = e = 0.0
    x = xf
    fx = yield x
    num = 1
    fu = np.inf
    ffulc = fnfc = fx
    xm = 0.5 * (a + b)
    tol1 = sqrt_eps * np.abs(xf) + xatol / 3.0
    tol2 = 2.0 * tol1
    while np.abs(xf - xm) > (tol2 - 0.5 * (b - a)):
        golden = 1
        if np.abs(e) > tol1:
            golden = 0
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = np.abs(q)
            r = e
            e = rat
            if (np.abs(p) < np.abs(0.5 * q * r)) and (p > q * (a - xf)) and (p < q * (b - xf)):
                rat = (p + 0.0) / q
                x = xf + rat
                if ((x - a) < tol2) or ((b - x) < tol2):
                    si = np.sign(xm - xf) + ((xm - xf) == 0)
                    rat = tol1 * si
            else:
                golden = 1
        if golden:
            e = a - xf if xf >= xm else b - xf
            rat = golden_mean * e
        si = np.sign(rat) + (rat == 0)
        x = xf + si * np.maximum(np.abs(rat), tol1)
        fu = yield x
        num += 1
        if fu <= fx:
            if x >= xf:
                a = xf
            else:
                b = xf
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
            else:
                b = x
            if (fu <= fnfc) or (nfc == xf):
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
            elif (fu <= ffulc) or (fulc == xf) or (fulc == nfc):
                fulc, ffulc = x, fu
        xm = 0.5 * (a + b)
        tol1 = sqrt_eps * np.abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= maxiter:
            flag = 1
            break
    if np.isnan(xf) or np.isnan(fx) or np.isnan(fu):
        flag = 2
    return dict(x=float(xf), fun=float(fx), nfev=num, status=flag)


def _kept_knots(cbv_time, cbvs, gap_indicators):
    """The checks of ``interpolate_cbvs`` -> (knot times, knot values (Nk, K)) without the gap-flagged cadences."""
    x = np.asarray(cbv_time, dtype=np.float64)
    y = np.asarray(cbvs, dtype=np.float64)
    if x.ndim != 1 or y.ndim != 2 or y.shape[0] != x.size:
        raise ValueError("cbv_time must be 1-D and cbvs 2-D with one row per CBV cadence (got %s and %s)" % (x.shape, y.shape))
    if y.shape[1] < 1:
        raise ValueError("cbvs needs at least one column")
    if gap_indicators is not None:
        gap = np.asarray(gap_indicators)
        if gap.shape != x.shape or (gap.dtype != np.bool_ and gap.dtype != np.uint8):
            raise ValueError("gap_indicators must be a bool array with one entry per CBV cadence")
        x, y = x[gap == 0], y[gap == 0]
    if x.size < 2:
        raise ValueError("interpolation needs at least 2 CBV cadences that are not gap-flagged (got %d)" % x.size)
    if not np.all(np.isfinite(x)) or np.any(np.diff(x) <= 0):
        raise ValueError("the times of the CBV cadences that are not gap-flagged must be finite and strictly increasing")
    if not np.all(np.isfinite(y)):
        raise ValueError("the basis vectors must be finite at every cadence that is not gap-flagged")
    return x, y


def pchip_slopes(x, y):
    """The derivatives ``scipy.interpolate.PchipInterpolator(x, y, axis=0)`` uses at its knots (scipy
    interpolate/_cubic.py ``_find_derivatives`` / ``_edge_case``): x (Nx,) strictly increasing, y (Nx, K) -> (Nx, K)."""
    h = np.diff(x)[:, None]
    m = np.diff(y, axis=0) / h
    d = np.zeros_like(y)
    if x.size == 2:
        d[0] = d[1] = m[0]
        return d
    flat = (np.sign(m[1:]) != np.sign(m[:-1])) | (m[1:] == 0) | (m[:-1] == 0)
    w1, w2 = 2 * h[1:] + h[:-1], h[1:] + 2 * h[:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        whmean = (w1 / m[:-1] + w2 / m[1:]) / (w1 + w2)
        d[1:-1] = np.where(flat, 0.0, 1.0 / whmean)

    def edge(h0, h1, m0, m1):
        e = ((2 * h0 + h1) * m0 - h0 * m1) / (h0 + h1)
        steep = (np.sign(m0) != np.sign(m1)) & (np.abs(e) > 3.0 * np.abs(m0))
        return np.where(np.sign(e) != np.sign(m0), 0.0, np.where(steep, 3.0 * m0, e))

    d[0] = edge(h[0], h[1], m[0], m[1])
    d[-1] = edge(h[-1], h[-2], m[-1], m[-2])
    return d


def interpolate_cbvs(cbv_time, cbvs, time, gap_indicators=None, extrapolate=False):
    """``CotrendingBasisVectors.interpolate(lc, extrapolate)`` on arrays (reference cbvcorrector.py: every basis vector
    through ``scipy.interpolate.PchipInterpolator`` with the cadences that are not gap-flagged as knots, evaluated at the
    light curve's times), restated in numpy so the product interpreter needs no scipy: ``cbvs`` (Nx, K) at ``cbv_time``
    (Nx,) -> (len(time), K).  A time outside the knots' span (or not finite) gives NaN unless ``extrapolate``, which
    continues the first / last cubic as scipy does.  A time bit-equal to a knot returns that knot's values bit for bit.
    This is the host mirror of ``lk_pchip_interp_batch`` (csrc/interp.hip): same interval, same coefficients, same Horner
    form."""
    x, y = _kept_knots(cbv_time, cbvs, gap_indicators)
    t = np.asarray(time, dtype=np.float64)
    if t.ndim != 1:
        raise ValueError("time must be 1-D")
    d = pchip_slopes(x, y)
    i = np.clip(np.searchsorted(x, t, side="right") - 1, 0, x.size - 2)
    dx = (x[i + 1] - x[i])[:, None]
    s = (t - x[i])[:, None]
    sl = (y[i + 1] - y[i]) / dx
    tt = (d[i] + d[i + 1] - 2 * sl) / dx
    c0, c1 = tt / dx, (sl - d[i]) / dx - tt
    with np.errstate(invalid="ignore", over="ignore"):
        out = y[i] + s * (d[i] + s * (c1 + s * c0))
    last = t == x[-1]
    out[last] = y[-1]
    if not extrapolate:
        out[~((t >= x[0]) & (t <= x[-1]))] = np.nan
    return out


class BoundedBrentBatch(object):
    """``minimize_scalar_bounded`` as a stepper for B independent searches on one interval, run in lockstep: ``.x`` is the
    next abscissa of every search (float64[B]), ``.tell(f)`` takes the B objective values there, ``.done`` (bool[B]) says
    which searches have ended and ``.result()`` gives the arrays x, fun, nfev, status.  Each search visits exactly the
    abscissae the scalar function would, given the same values (B scalar states: the searches share nothing).  A finished
    search keeps its final ``xf`` in ``.x``; whatever ``tell`` is given for it is ignored."""

    def __init__(self, bounds, B, xatol=1e-5, maxiter=500):
        x1, x2 = float(bounds[0]), float(bounds[1])
        if not (np.isfinite(x1) and np.isfinite(x2)):
            raise ValueError("Optimization bounds must be finite scalars.")
        if x1 > x2:
            raise ValueError("The lower bound exceeds the upper bound.")
        if int(B) < 1:
            raise ValueError("B must be >= 1 (got %r)" % (B,))
        self._steps = [_bounded_brent_steps(x1, x2, xatol, maxiter) for _ in range(int(B))]
        self._results = [None] * int(B)
        self.x = np.array([float(next(g)) for g in self._steps], dtype=np.float64)
        self.done = np.zeros(int(B), dtype=bool)

    def tell(self, f):
        f = np.asarray(f, dtype=np.float64)
        if f.shape != self.x.shape:
            raise ValueError("tell() takes one objective value per search, shape %s (got %s)" % (self.x.shape, f.shape))
        for b, g in enumerate(self._steps):
            if self.done[b]:
                continue
            try:
                self.x[b] = g.send(f[b])
            except StopIteration as stop:
                self._results[b] = stop.value
                self.done[b] = True
                self.x[b] = stop.value["x"]

    def result(self):
        if not self.done.all():
            raise ValueError("%d of the %d searches have not ended" % ((~self.done).sum(), len(self.done)))
        r = self._results
        return dict(x=np.array([v["x"] for v in r], dtype=np.float64), fun=np.array([v["fun"] for v in r], dtype=np.float64),
                    nfev=np.array([v["nfev"] for v in r], dtype=np.int64), status=np.array([v["status"] for v in r], dtype=np.int64))


def cbv_index_list(cbv_indices, n_vectors):
    """Basis-vector numbers as ``CBVCorrector`` takes them -> int array: 1-based, "ALL" = every vector, numbers outside
    1..n_vectors dropped."""
    if isinstance(cbv_indices, str) and cbv_indices == "ALL":
        cbv_indices = np.arange(1, n_vectors + 1)
    return np.array([i for i in np.asarray(cbv_indices) if 1 <= i <= n_vectors], dtype=int)


class CBVCorrector(RegressionCorrector):
    def __init__(self, lc, cbvs, cbv_type="SingleScale"):
        """``cbvs``: float array (n_cadences, n_vectors), column j = basis vector number j + 1 on the cadences of lc."""
        super(CBVCorrector, self).__init__(lc)
        self.cbvs = np.asarray(cbvs, dtype=np.float64)
        if self.cbvs.ndim != 2 or self.cbvs.shape[0] != len(lc.time):
            raise ValueError("cbvs must have one row per cadence of the light curve")
        self.cbv_type = cbv_type
        self.alpha = None
        self.neighbor_flux = None          # (n_cadences, n_neighbours) for the under-fitting metric, see set_neighbors
        self.optimization_params = None
        self.over_fitting_score = None
        self.under_fitting_score = None

    def _collection(self, cbv_indices, ext_dm):
        mats = []
        if cbv_indices is not None:
            idx = cbv_index_list(cbv_indices, self.cbvs.shape[1])
            mats.append(DesignMatrix(self.cbvs[:, idx - 1], columns=["VECTOR_%d" % i for i in idx], name=self.cbv_type))
        if ext_dm is not None:
            if not isinstance(ext_dm, DesignMatrix):
                raise ValueError("ext_dm must be a DesignMatrix")
            if ext_dm.shape[0] != len(self.lc.flux):
                raise ValueError("ext_dm must contain the same number of cadences as lc.flux")
            mats.append(ext_dm)
        if not mats:
            raise ValueError("nothing to fit: pass cbv_indices and/or ext_dm")
        mats.append(DesignMatrix(np.ones(len(self.lc.time)), columns=["Constant"], name="Constant"))
        return DesignMatrixCollection(mats)

    def correct_gaussian_prior(self, cbv_indices=np.arange(1, 9), alpha=1e-20, ext_dm=None, cadence_mask=None, **kwargs):
        dmc = self._collection(cbv_indices, ext_dm)
        sigma = None if alpha == 0.0 else np.median(self.lc.flux_err) / np.sqrt(np.abs(alpha))
        for dm in dmc.matrices:
            dm.prior_sigma = np.ones(dm.shape[1]) * (np.inf if sigma is None else sigma)
        self.alpha = alpha
        return self.correct_regressioncorrector(dmc, cadence_mask=cadence_mask, **kwargs)

    def correct_regressioncorrector(self, design_matrix_collection, **kwargs):
        """Pass-through to ``RegressionCorrector.correct`` (reference cbvcorrector.py:494-500); ``CBVCorrector.correct``
        itself is the goodness-metric optimisation below."""
        return super(CBVCorrector, self).correct(design_matrix_collection, **kwargs)

    # ------------------------------------------------------------------------------------------------ goodness metrics
    def set_neighbors(self, neighbor_flux):
        """Flux of the neighbouring targets on this light curve's cadences, shape (n_cadences, n_neighbours).  The
        reference downloads them from MAST inside ``under_fitting_metric`` (metrics.py:274-330, control plane); here the
        caller hands them over once."""
        nf = np.asarray(neighbor_flux, dtype=np.float64)
        if nf.ndim != 2 or nf.shape[0] != len(self.lc.time):
            raise ValueError("neighbor_flux must be (n_cadences, n_neighbours)")
        self.neighbor_flux = nf

    def over_fitting_metric(self, n_samples=10, device=0):
        """cbvcorrector.py:502-533 -> metrics.overfit_metric_lombscargle on the unmasked cadences."""
        if self.corrected_lc is None:
            return None
        cm = self.cadence_mask
        return overfit_metric_lombscargle(self.lc[cm], self.corrected_lc[cm], n_samples=n_samples, device=device)

    def under_fitting_metric(self):
        """cbvcorrector.py:535-637 -> metrics.underfit_metric_neighbors; needs ``set_neighbors`` first."""
        if self.corrected_lc is None:
            raise Exception("A corrected light curve does not exist, please run correct first")
        if self.neighbor_flux is None:
            raise ValueError("under_fitting_metric needs the neighbouring targets: call set_neighbors(flux) first "
                             "(the reference downloads them from MAST)")
        cm = self.cadence_mask
        return underfit_metric_neighbors(self.corrected_lc[cm], self.neighbor_flux[cm])

    def _goodness_metric_obj_fun(self, alpha, device=0):
        """cbvcorrector.py:781-854: ridge fit at ``alpha``, then -(over + under) with the leaky-ReLU easing above the
        target scores."""
        op = self.optimization_params
        sigma = np.median(self.lc.flux_err) / np.sqrt(np.abs(alpha))
        for dm in self._dmc_opt.matrices:
            dm.prior_sigma = np.ones(dm.shape[1]) * sigma
        self.correct_regressioncorrector(self._dmc_opt, cadence_mask=op["cadence_mask"], device=device)
        over = self.over_fitting_metric(n_samples=op["over_metric_nSamples"], device=device) \
            if op["target_over_score"] > 0 else 1.0
        under = self.under_fitting_metric() if op["target_under_score"] > 0 else 1.0
        return -(_leaky(over, op["target_over_score"]) + _leaky(under, op["target_under_score"]))

    def correct(self, cbv_type=None, cbv_indices=np.arange(1, 9), ext_dm=None, cadence_mask=None,
                alpha_bounds=(1e-4, 1e4), target_over_score=0.5, target_under_score=0.5, max_iter=100, device=0):
        """``CBVCorrector.correct`` (reference cbvcorrector.py:397-500): bounded Brent search for the ridge penalty alpha
        that maximises the goodness metrics, a final fit at the optimum, then the scores with n_samples=10.
        ``cbv_type`` is accepted for signature compatibility (this mirror holds ONE set of basis vectors);
        ``cbv_indices=None`` fits ``ext_dm`` only, like the reference with ``do_not_load_cbvs``.  A score with a
        non-positive target is skipped (and reported as -1), as in the reference."""
        self._dmc_opt = self._collection(cbv_indices, ext_dm)
        self.optimization_params = {"alpha_bounds": list(alpha_bounds), "target_over_score": target_over_score,
                                    "target_under_score": target_under_score, "max_iter": max_iter,
                                    "cadence_mask": cadence_mask, "over_metric_nSamples": 1}
        res = minimize_scalar_bounded(lambda a: self._goodness_metric_obj_fun(a, device=device), alpha_bounds,
                                      maxiter=max_iter)
        self._goodness_metric_obj_fun(res["x"], device=device)          # minimize_scalar does not end on the optimum
        self.over_fitting_score = self.over_fitting_metric(n_samples=10, device=device) if target_over_score > 0 else -1.0
        self.under_fitting_score = self.under_fitting_metric() if target_under_score > 0 else -1.0
        self.alpha = res["x"]
        self.optimization_result = res
        return self.corrected_lc

    def goodness_scan(self, alphas, cbv_indices=np.arange(1, 9), ext_dm=None, cadence_mask=None, n_samples=1,
                      device=0):
        """The goodness objective's ingredients for MANY ridge penalties at once: ONE batched regression (the same
        light curve and design matrix with len(alphas) different prior widths) and ONE batched periodogram call for all
        the over-fitting metrics.  Returns dict(alpha, over_fitting[len(alphas)], under_fitting (or None),
        corrected_flux[len(alphas), n_cadences]).  The noise draws follow the reference's order per alpha."""
        alphas = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
        dmc = self._collection(cbv_indices, ext_dm)
        n, K, A = len(self.lc.time), dmc.X.shape[1], len(alphas)
        cm = np.ones(n, bool) if cadence_mask is None else np.asarray(cadence_mask, dtype=bool)
        sig = np.median(self.lc.flux_err) / np.sqrt(np.abs(alphas))
        err = None if np.all(~np.isfinite(self.lc.flux_err)) else np.tile(self.lc.flux_err, A)
        res = _capi.regress_batch(np.tile(dmc.X, (A, 1)), np.tile(self.lc.flux, A), np.arange(A + 1) * n, err=err,
                                  cadence_mask=np.tile(cm, A), prior_mu=np.zeros((A, K)),
                                  prior_sigma=np.repeat(sig[:, None], K, axis=1), device=device)
        corrected = self.lc.flux[None, :] - res["model"].reshape(A, n)
        orig = self.lc[cm]
        cors = []
        for a in range(A):
            c = self.lc.copy()
            c.flux = corrected[a]
            cors.append(c[cm])
        over = overfit_metric_lombscargle_batch(orig, cors, n_samples=n_samples, device=device)
        under = None
        if self.neighbor_flux is not None:
            under = np.array([underfit_metric_neighbors(c, self.neighbor_flux[cm]) for c in cors])
        return dict(alpha=alphas, over_fitting=over, under_fitting=under, corrected_flux=corrected,
                    coefficients=res["coefficients"])


def _leaky(metric, target, leak=0.01):
    """cbvcorrector.py:838-850: above the target the metric only counts with 1 % of its excess."""
    if target > 0 and metric >= target:
        return target + leak * (metric - target)
    return metric
