"""Cotrending of a resident batch on one shared design matrix: ``regression_correct`` / ``cbv_correct``, the under- and
over-fitting goodness metrics, ``cbv_goodness_scan`` and the per-target ridge search ``cbv_correct_optimized``.

``CotrendMixin`` holds the public methods; ``DeviceLightCurveBatch`` (device.py) inherits it.  A batch comes in one of two
layouts: UNIFORM (one cadence count ``N``, row j of the matrix is cadence j of every target) or ROWS (ragged offsets, every
cadence names its row of the matrix; ``cadenceno=``).  ``_UniformLayout`` / ``_RowsLayout`` own what a scan or a search keeps
resident for their route and call that route's C entry points under the same method names; ``_goodness_scan`` and
``_ridge_search`` are written once on top of them and make no device call of their own."""
import ctypes

import numpy as np

from . import _capi
from .devmem import DeviceBuffer, _off_ptr, _p, _upload, _vp


class CotrendMixin(object):
    """The cotrending methods of ``DeviceLightCurveBatch`` (they use its columns, offsets, ``_new`` / ``_carry`` / ``select``)."""

    def _uniform_n(self, rows, what):
        """The one cadence count of the batch, checked against the ``rows`` of the shared design matrix unless ``rows`` is None
        (no device call)."""
        counts = np.diff(self.n_off)
        if len(counts) == 0:
            raise ValueError("%s needs at least one light curve" % what)
        if counts.min() != counts.max():
            if rows is None:
                raise ValueError("%s needs one cadence count for every target: this batch has between %d and %d cadences per target"
                                 % (what, counts.min(), counts.max()))
            raise ValueError("%s needs one cadence count for every target: this batch has between %d and %d cadences per target "
                             "and the design matrix has %d rows (regression_correct_batch takes ragged batches)"
                             % (what, counts.min(), counts.max(), rows))
        N = int(counts[0])
        if rows is not None and rows != N:
            raise ValueError("%s: the design matrix has %d rows, the light curves have %d cadences" % (what, rows, N))
        return N

    def regression_correct(self, X, prior_mu=None, prior_sigma=None, cadence_mask=None, sigma=5, niters=5, to_host=False, rows=None,
                           cadenceno=None, knot_time=None, extrapolate=False, knot_keep=None, design_slab_mb=4096):
        """``RegressionCorrector(lc).correct(X, cadence_mask, sigma, niters)`` (reference regressioncorrector.py:191-279,
        ``propagate_errors=False``) for every target of the batch on ONE shared design matrix: ``X`` is a host array (N, K),
        K <= 64, or a ``DesignMatrix`` / ``DesignMatrixCollection`` (its own priors go to every target unless ``prior_mu`` /
        ``prior_sigma``, broadcastable to (B, K), are given).  X is uploaded once; no (B N) x K matrix exists.  The corrected
        flux is flux - model, formed on the device; flux_err is unchanged.  ``cadence_mask``: bool (B, N), True = used in the
        fit.  ``to_host=False`` -> (``DeviceLightCurveBatch``, ``DeviceBuffer`` of the B x N outlier bytes, ``DeviceBuffer``
        of the B x K coefficients), nothing synchronised after the input check; ``to_host=True`` -> (corrected[B, N],
        outlier[B, N] bool, coefficients[B, K]).

        A RAGGED batch (``from_fits``, ``remove_nans``, ``remove_outliers``, ``select``) is fitted on the same one matrix when
        the call says which row of ``X`` each cadence uses: ``cadenceno`` = the integer cadence numbers of the Nx rows of ``X``,
        strictly increasing, matched against the batch's own ``d_cadenceno`` column (``CotrendingBasisVectors.align``: a
        cadence of a target that is not on the grid is dropped first, the count per target goes to
        ``meta[b]["CADENCES_NOT_ON_GRID"]`` of the result; a grid row that no target has carries no weight), or ``rows`` =
        int (sum n,), per target strictly increasing indices into the rows of ``X``.  Per target the numerics are
        ``RegressionCorrector.correct`` on ``X[rows_b]``.  ``cadence_mask`` is then ragged: bool (sum n,) over the cadences of
        this batch, or a ``DeviceBuffer`` of that many bytes.  The result is the same triple on the batch's own offsets
        (outlier bytes (sum n,)); ``to_host=True`` -> (list of corrected[n_b], list of outlier[n_b] bool, coefficients[B, K]).

        The third route, for light curves whose cadences are NOT rows of ``X`` (another cadence length, binned light curves,
        times that differ by seconds, no cadence numbers): ``knot_time`` = the times of the Nx rows of ``X``, float (Nx,),
        strictly increasing where ``knot_keep`` (bool (Nx,), None = everywhere; the reference's ``~gap_indicators``) is
        true.  Every column of ``X`` is then interpolated to each target's own times as ``CotrendingBasisVectors.interpolate``
        does (``scipy.interpolate.PchipInterpolator`` on the kept rows; ``lk_pchip_interp_batch_dev``) and every target is
        fitted on its own interpolated matrix (``lk_regress_batch_dev``; any K that call takes).  Not to be combined with
        ``rows`` / ``cadenceno``.  ``extrapolate=False``: a cadence outside the kept knots' span (or with a time that is not
        finite) is dropped before the fit, exactly as an off-grid cadence is, and counted in
        ``meta[b]["CADENCES_OUTSIDE_CBVS"]`` of the result; a target left with no cadence is a ``ValueError`` naming it.
        ``extrapolate=True``: nothing is dropped, the first / last cubic is continued as scipy does.  ``cadence_mask`` and
        the results are ragged as above.  The interpolated matrices are 8 K (sum n) bytes: whole targets are fitted in
        groups whose matrices stay under ``design_slab_mb`` MiB (a target's result does not depend on the grouping, bit
        for bit)."""
        Xa, mu, sg = _design_arrays(X, prior_mu, prior_sigma)
        if knot_time is not None:
            if rows is not None or cadenceno is not None:
                raise ValueError("regression_correct: `knot_time` interpolates X to the targets' own times; it cannot be combined "
                                 "with `rows` / `cadenceno`")
            src, d_cm, keep, knots = self._interp_front(Xa, knot_time, knot_keep, extrapolate, cadence_mask, "regression_correct")
            d_mu, d_sg = src._upload_priors(mu, sg, Xa.shape[1], keep)
            return src._regress_interp(knots, False, extrapolate, d_mu, d_sg, d_cm, sigma, niters, to_host, keep, design_slab_mb)
        if knot_keep is not None or extrapolate:
            raise ValueError("regression_correct: `knot_keep` / `extrapolate` belong to the interpolated route: pass `knot_time`")
        if rows is not None or cadenceno is not None:
            src, d_rows, d_cm, keep = self._aligned(Xa.shape[0], rows, cadenceno, cadence_mask, "regression_correct")
            d_mu, d_sg = src._upload_priors(mu, sg, Xa.shape[1], keep)
            return src._regress_shared_rows(Xa, d_rows, d_mu, d_sg, d_cm, sigma, niters, to_host, keep)
        N = self._uniform_n(Xa.shape[0], "regression_correct")
        keep = []
        d_mu, d_sg = self._upload_priors(mu, sg, Xa.shape[1], keep)
        return self._regress_shared(Xa, N, d_mu, d_sg, cadence_mask, sigma, niters, to_host, keep)

    def _upload_priors(self, mu, sg, K, keep):
        """``prior_mu`` / ``prior_sigma`` broadcast to (B, K) and uploaded -> (d_mu, d_sg); (None, None) without priors."""
        if mu is None:
            return None, None
        d_mu, k1 = _upload(self.handle, np.broadcast_to(mu, (len(self), K)), self.stream)
        d_sg, k2 = _upload(self.handle, np.broadcast_to(sg, (len(self), K)), self.stream)
        keep += [k1, k2]
        return d_mu, d_sg

    def _aligned(self, Nx, rows, cadenceno, cadence_mask, what):
        """The ragged route's front end -> (batch to fit, d_rows, d_cm, keep).  Every check that needs no device comes first.
        With ``cadenceno`` the rows come from ``lk_align_rows_batch_dev``; when a target has cadences that are not on the grid
        the batch (and a ragged ``cadence_mask``) is ``select``-ed down to the matched cadences and aligned again."""
        n, B = self.n_cadences, len(self)
        if rows is not None and cadenceno is not None:
            raise ValueError("%s: pass `rows` or `cadenceno`, not both" % what)
        if B == 0 or n == 0:
            raise ValueError("%s needs at least one light curve with cadences" % what)
        mask = _RaggedMask(self, cadence_mask, "with `rows` / `cadenceno`", what)
        if rows is not None:
            r = _cadenceno_array(rows, n, "rows")
            if r.size and (r.min() < 0 or r.max() >= Nx):
                raise ValueError("%s: rows must be indices into the %d rows of the design matrix" % (what, Nx))
        else:
            grid = _cadenceno_array(cadenceno, Nx, "cadenceno (one per row of the design matrix)")
            if np.any(np.diff(grid) <= 0):
                raise ValueError("%s: the grid's cadence numbers must be strictly increasing" % what)
            if getattr(self, "d_cadenceno", None) is None:
                raise ValueError("%s(cadenceno=) needs a batch that carries cadence numbers: from_fits of files with a CADENCENO "
                                 "column, or from_arrays(..., cadenceno=)" % what)
        h, st, keep = self.handle, _vp(self.stream or None), []
        if rows is not None:
            d_rows, k = _upload(h, r, self.stream, np.int32)
            keep.append(k)
            src = self
        else:
            d_grid, k = _upload(h, grid, self.stream, np.int32)
            keep += [k, d_grid]
            src, dropped = self, np.zeros(B, dtype=np.int64)
            d_rows = DeviceBuffer(h, n * 4)
            try:
                _capi._check(_capi._lib.lk_align_rows_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(self.d_cadenceno.ptr), Nx,
                                                                _vp(d_grid.ptr), _vp(d_rows.ptr), None, st))
            except ValueError as exc:
                if "not on the grid" not in str(exc):
                    raise
                off_grid = d_rows.download(np.int32, n, stream=self.stream) < 0       # (rows is written before the call fails)
                dropped = np.diff(np.concatenate([[0], np.cumsum(off_grid, dtype=np.int64)])[self.n_off])
                src = self.select(off_grid, invert=True)
                mask.drop(off_grid)
                d_rows = DeviceBuffer(h, max(src.n_cadences, 1) * 4)
                _capi._check(_capi._lib.lk_align_rows_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(src.d_cadenceno.ptr), Nx,
                                                                _vp(d_grid.ptr), _vp(d_rows.ptr), None, st))
            if src is self:
                src = self._carry(self._new(self.d_time, self.d_flux, self.d_flux_err, self.n_off, nan_free=self.nan_free,
                                            is_sorted=self.is_sorted))
            for m, c in zip(src.meta, dropped):
                m["CADENCES_NOT_ON_GRID"] = int(c)
        return src, d_rows, mask.on_device(keep), keep

    def _interp_front(self, Ya, knot_time, knot_keep, extrapolate, cadence_mask, what):
        """The interpolated route's front end -> (batch to fit, d_cm, keep, (d_x, d_Y, d_keep, Nx, K)).  Every check that
        needs no device comes first.  Without ``extrapolate`` the inside bytes come from ``lk_pchip_interp_batch_dev`` (which
        also checks the knots) and the batch (and ``cadence_mask``) is ``select``-ed down to the cadences inside the span."""
        n, B = self.n_cadences, len(self)
        x = np.asarray(knot_time)
        if x.ndim != 1 or x.shape[0] != Ya.shape[0] or not (np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.integer)):
            raise ValueError("%s: the knot times must be a real array of shape (%d,), one per row of the matrix (got %s of shape %s)"
                             % (what, Ya.shape[0], x.dtype, x.shape))
        x = np.ascontiguousarray(x, dtype=np.float64)
        kk = None
        if knot_keep is not None:
            kk = np.asarray(knot_keep)
            if kk.shape != x.shape or (kk.dtype != np.bool_ and kk.dtype != np.uint8):
                raise ValueError("%s: the knot mask must be a bool array of shape (%d,) (got %s of shape %s)"
                                 % (what, x.size, kk.dtype, kk.shape))
            kk = np.ascontiguousarray(kk != 0, dtype=np.uint8)
        if int(x.size if kk is None else kk.sum()) < 2:
            raise ValueError("%s: interpolation needs at least 2 knots that are kept" % what)
        if B == 0 or n == 0:
            raise ValueError("%s needs at least one light curve with cadences" % what)
        mask = _RaggedMask(self, cadence_mask, "on the interpolated route", what)
        h, st, keep = self.handle, _vp(self.stream or None), []
        d_x, k1 = _upload(h, x, self.stream)
        d_Y, k2 = _upload(h, Ya, self.stream)
        keep += [k1, k2]
        d_keep = None
        if kk is not None:
            d_keep, k3 = _upload(h, kk, self.stream, np.uint8)
            keep.append(k3)
        knots = (d_x, d_Y, d_keep, Ya.shape[0], Ya.shape[1])
        src, dropped = self, np.zeros(B, dtype=np.int64)
        if not extrapolate:
            d_in = DeviceBuffer(h, n)
            _capi._check(_capi._lib.lk_pchip_interp_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), Ya.shape[0],
                                                              Ya.shape[1], _vp(d_x.ptr), _vp(d_Y.ptr),
                                                              _p(d_keep), 0, 0, None,
                                                              _vp(d_in.ptr), st))
            outside = d_in.download(np.uint8, n, stream=self.stream) == 0
            if outside.any():
                dropped = np.diff(np.concatenate([[0], np.cumsum(outside, dtype=np.int64)])[self.n_off])
                empty = np.flatnonzero(dropped == np.diff(self.n_off))
                if empty.size:
                    raise ValueError("%s: target %d has no cadence inside the span of the knots (extrapolate=True keeps them)"
                                     % (what, int(empty[0])))
                src = self.select(d_in)
                mask.drop(outside)
        if np.any(np.diff(src.n_off) == 0):
            raise ValueError("%s: target %d has no cadence" % (what, int(np.flatnonzero(np.diff(src.n_off) == 0)[0])))
        if src is self:
            src = self._carry(self._new(self.d_time, self.d_flux, self.d_flux_err, self.n_off, nan_free=self.nan_free,
                                        is_sorted=self.is_sorted))
        for m, c in zip(src.meta, dropped):
            m["CADENCES_OUTSIDE_CBVS"] = int(c)
        return src, mask.on_device(keep), keep, knots

    def _regress_interp(self, knots, append_constant, extrapolate, d_mu, d_sg, d_cm, sigma, niters, to_host, keep, design_slab_mb):
        """Interpolate and fit, whole targets in groups whose design matrices fit ``design_slab_mb``; one slab, reused."""
        d_x, d_Y, d_keep, Nx, K = knots
        h, B, n, st = self.handle, len(self), self.n_cadences, _vp(self.stream or None)
        Kout = K + int(bool(append_constant))
        budget = int(float(design_slab_mb) * (1 << 20)) // (8 * Kout)        # cadences per group
        if budget < 1:
            raise ValueError("design_slab_mb=%r holds not one row of the design matrix" % (design_slab_mb,))
        groups, b0 = [], 0
        while b0 < B:
            b1 = b0 + 1
            while b1 < B and self.n_off[b1 + 1] - self.n_off[b0] <= budget and b1 - b0 < 65535:
                b1 += 1
            groups.append((b0, b1))
            b0 = b1
        d_slab = DeviceBuffer(h, 8 * Kout * int(max(self.n_off[b1] - self.n_off[b0] for b0, b1 in groups)))
        d_w, d_model, d_corr, d_outl = DeviceBuffer(h, B * Kout * 8), DeviceBuffer(h, n * 8), DeviceBuffer(h, n * 8), DeviceBuffer(h, n)
        lib = _capi._lib
        for b0, b1 in groups:
            o = int(self.n_off[b0])
            off = np.ascontiguousarray(self.n_off[b0:b1 + 1] - o)
            _capi._check(lib.lk_pchip_interp_batch_dev(h._h, b1 - b0, _off_ptr(off), _p(self.d_time, 8 * o), Nx, K, _vp(d_x.ptr),
                                                       _vp(d_Y.ptr), _p(d_keep, 0), int(bool(extrapolate)), int(bool(append_constant)),
                                                       _vp(d_slab.ptr), None, st))
            _capi._check(lib.lk_regress_batch_dev(h._h, b1 - b0, _off_ptr(off), Kout, _vp(d_slab.ptr), _p(self.d_flux, 8 * o),
                                                  _p(self.d_flux_err, 8 * o), _p(d_cm, o), _p(d_mu, 8 * Kout * b0),
                                                  _p(d_sg, 8 * Kout * b0), float(sigma), int(niters), _p(d_w, 8 * Kout * b0),
                                                  _p(d_model, 8 * o), _p(d_outl, o), st))
        _capi._check(lib.lk_subtract_f64_dev(h._h, n, _vp(self.d_flux.ptr), _vp(d_model.ptr), _vp(d_corr.ptr), st))
        return self._regress_result(None, Kout, d_corr, d_outl, d_w, to_host, keep + [d_x, d_Y, d_keep, d_slab, d_cm, d_mu, d_sg, d_model])

    def _regress_shared_rows(self, Xa, d_rows, d_mu, d_sg, d_cm, sigma, niters, to_host, keep, resident=None):
        """``resident``: d_X already in HBM (a search that fits the same matrix many times uploads it once)."""
        h, B, K, n = self.handle, len(self), Xa.shape[1], self.n_cadences
        if resident is not None:
            d_X = resident
        else:
            d_X, k = _upload(h, Xa, self.stream)
            keep.append(k)
        d_w, d_model, d_corr, d_outl = DeviceBuffer(h, B * K * 8), DeviceBuffer(h, n * 8), DeviceBuffer(h, n * 8), DeviceBuffer(h, n)
        _capi._check(_capi._lib.lk_regress_shared_rows_batch_dev(
            h._h, B, _off_ptr(self.n_off), _vp(d_rows.ptr), Xa.shape[0], K, _vp(d_X.ptr), _vp(self.d_flux.ptr),
            _p(self.d_flux_err), _p(d_cm), _p(d_mu), _p(d_sg), float(sigma), int(niters), _vp(d_w.ptr), _vp(d_model.ptr),
            _vp(d_outl.ptr), None, _vp(self.stream or None)))
        _capi._check(_capi._lib.lk_subtract_f64_dev(h._h, n, _vp(self.d_flux.ptr), _vp(d_model.ptr), _vp(d_corr.ptr),
                                                    _vp(self.stream or None)))
        return self._regress_result(None, K, d_corr, d_outl, d_w, to_host, keep + [d_X, d_rows, d_cm, d_mu, d_sg, d_model])

    def cbv_correct(self, cbvs, cbv_indices=np.arange(1, 9), alpha=1e-20, ext_dm=None, cadence_mask=None, sigma=5, niters=5,
                    to_host=False, cadenceno=None, cbv_time=None, gap_indicators=None, extrapolate=False, design_slab_mb=4096):
        """``CBVCorrector(lc, cbvs).correct_gaussian_prior(cbv_indices, alpha, ext_dm, cadence_mask)`` (reference
        cbvcorrector.py:333-395) for every target of the batch: columns [cbvs[:, idx - 1] | ext_dm | 1] shared by all targets
        (``cbvs``: (N, n_vectors), column j = basis vector j + 1; indices 1-based, out-of-range ones dropped, "ALL" accepted),
        prior_mu = 0 and ONE ridge width per target, median(flux_err_b) / sqrt(|alpha|), taken on the device; ``alpha == 0``:
        no prior.  ``alpha`` may also be an array-like of B finite, non-zero penalties, one per target (8 bytes per target go
        up; row b is what the scalar call at ``alpha[b]`` gives, bit for bit); a zero inside an array is a ``ValueError``:
        "no prior" stays the scalar ``alpha == 0.0``.  Returns what ``regression_correct`` returns.  ``cadenceno``: the cadence
        numbers of the rows of ``cbvs``; the batch may then be ragged and is matched by its own cadence numbers, exactly as
        ``regression_correct(cadenceno=)`` (the ridge width is the median over the target's own matched cadences).

        ``cbv_time``: the times of the rows of ``cbvs`` -> ``CBVCorrector(lc, interpolate_cbvs=True, extrapolate_cbvs=
        extrapolate)``: the selected vectors are interpolated to every target's own times (``regression_correct(knot_time=)``;
        ``gap_indicators``: bool (Nx,), True = a CBV cadence that is no knot, the reference's ``cbvs.gap_indicators``), the
        constant column is written with them, and the batch needs neither one cadence count nor cadence numbers.  Not to be
        combined with ``cadenceno``; ``ext_dm`` lives on the CBV cadences and is not interpolated: a ``ValueError``.  The
        ridge width is the median over the target's own cadences that are fitted (inside the CBVs' span unless ``extrapolate``);
        the dropped ones are counted in ``meta[b]["CADENCES_OUTSIDE_CBVS"]``."""
        if cbv_time is not None:
            if cadenceno is not None:
                raise ValueError("cbv_correct: `cbv_time` interpolates the basis vectors to the targets' own times; it cannot be "
                                 "combined with `cadenceno`")
            if ext_dm is not None:
                raise ValueError("cbv_correct(cbv_time=): `ext_dm` is not interpolated; put its columns on the targets' own "
                                 "cadences and use regression_correct_batch, or fit it on the cadence grid (cadenceno=)")
            if cbv_indices is None:
                raise ValueError("nothing to fit: pass cbv_indices")
            Ya = np.ascontiguousarray(_cbv_columns(cbvs, cbv_indices, None)[:, :-1])
            alphas = None if np.ndim(alpha) == 0 else _alpha_per_target(alpha, len(self))
            kk = None
            if gap_indicators is not None:
                gap = np.asarray(gap_indicators)
                if gap.shape != (Ya.shape[0],) or (gap.dtype != np.bool_ and gap.dtype != np.uint8):
                    raise ValueError("cbv_correct: gap_indicators must be a bool array of shape (%d,) (got %s of shape %s)"
                                     % (Ya.shape[0], gap.dtype, gap.shape))
                kk = gap == 0
            src, d_cm, keep, knots = self._interp_front(Ya, cbv_time, kk, extrapolate, cadence_mask, "cbv_correct")
            d_mu, d_sg = src._ridge_prior(None, Ya.shape[1] + 1, alpha, alphas, keep)
            return src._regress_interp(knots, True, extrapolate, d_mu, d_sg, d_cm, sigma, niters, to_host, keep, design_slab_mb)
        if gap_indicators is not None or extrapolate:
            raise ValueError("cbv_correct: `gap_indicators` / `extrapolate` belong to the interpolated route: pass `cbv_time`")
        Xa = _cbv_columns(cbvs, cbv_indices, ext_dm)
        if cadenceno is not None:
            alphas = None if np.ndim(alpha) == 0 else _alpha_per_target(alpha, len(self))
            src, d_rows, d_cm, keep = self._aligned(Xa.shape[0], None, cadenceno, cadence_mask, "cbv_correct")
            d_mu, d_sg = src._ridge_prior(None, Xa.shape[1], alpha, alphas, keep)
            return src._regress_shared_rows(Xa, d_rows, d_mu, d_sg, d_cm, sigma, niters, to_host, keep)
        N = self._uniform_n(Xa.shape[0], "cbv_correct")
        alphas = None if np.ndim(alpha) == 0 else _alpha_per_target(alpha, len(self))
        keep = []
        d_mu, d_sg = self._ridge_prior(N, Xa.shape[1], alpha, alphas, keep)
        return self._regress_shared(Xa, N, d_mu, d_sg, cadence_mask, sigma, niters, to_host, keep)

    def _ridge_prior(self, N, K, alpha, alphas, keep):
        """(prior_mu, prior_sigma) on the device for one scalar ``alpha`` (0: (None, None), no prior) or, when ``alphas`` is
        not None, for one checked penalty per target."""
        if alphas is None and alpha == 0.0:
            return None, None
        if getattr(self, "d_flux_err", None) is None:
            raise ValueError("cbv_correct with alpha != 0 needs flux errors (the ridge width is median(flux_err) / sqrt(|alpha|))")
        h, B, st = self.handle, len(self), _vp(self.stream or None)
        d_mu, d_sg = DeviceBuffer(h, B * K * 8), DeviceBuffer(h, B * K * 8)
        lib = _capi._lib
        if alphas is not None:
            d_alpha, k = _upload(h, alphas, self.stream)
            keep += [k, d_alpha]
        if N is None:       # ragged: the median over each target's own cadences
            if alphas is None:
                _capi._check(lib.lk_ridge_prior_rows_batch_dev(h._h, B, _off_ptr(self.n_off), K, _vp(self.d_flux_err.ptr), float(alpha),
                                                               _vp(d_mu.ptr), _vp(d_sg.ptr), st))
            else:
                _capi._check(lib.lk_ridge_prior_rows_alphas_batch_dev(h._h, B, _off_ptr(self.n_off), K, _vp(self.d_flux_err.ptr),
                                                                      _vp(d_alpha.ptr), _vp(d_mu.ptr), _vp(d_sg.ptr), st))
        elif alphas is None:
            _capi._check(lib.lk_ridge_prior_batch_dev(h._h, B, N, K, _vp(self.d_flux_err.ptr), float(alpha), _vp(d_mu.ptr),
                                                      _vp(d_sg.ptr), st))
        else:
            _capi._check(lib.lk_ridge_prior_alphas_batch_dev(h._h, B, N, K, _vp(self.d_flux_err.ptr), _vp(d_alpha.ptr),
                                                             _vp(d_mu.ptr), _vp(d_sg.ptr), st))
        return d_mu, d_sg

    def _regress_shared(self, Xa, N, d_mu, d_sg, cadence_mask, sigma, niters, to_host, keep, resident=None):
        """``resident``: (d_X, d_cm) already in HBM (a search that fits the same matrix many times uploads them once); then
        ``cadence_mask`` is not looked at."""
        h, B, K = self.handle, len(self), Xa.shape[1]
        if resident is not None:
            d_X, d_cm = resident
        else:
            d_cm = None
            if cadence_mask is not None:
                cm = np.ascontiguousarray(cadence_mask, dtype=np.uint8)
                if cm.shape != (B, N):
                    raise ValueError("cadence_mask must be (B, N) = %s (got %s)" % ((B, N), cm.shape))
                d_cm, k = _upload(h, cm, self.stream, np.uint8)
                keep.append(k)
            d_X, k = _upload(h, Xa, self.stream)
            keep.append(k)
        d_w, d_model, d_corr, d_outl = DeviceBuffer(h, B * K * 8), DeviceBuffer(h, B * N * 8), DeviceBuffer(h, B * N * 8), DeviceBuffer(h, B * N)
        _capi._check(_capi._lib.lk_regress_shared_batch_dev(
            h._h, B, N, K, _vp(d_X.ptr), _vp(self.d_flux.ptr), _p(self.d_flux_err), _p(d_cm), _p(d_mu), _p(d_sg), float(sigma),
            int(niters), _vp(d_w.ptr), _vp(d_model.ptr), _vp(d_outl.ptr), None, _vp(self.stream or None)))
        _capi._check(_capi._lib.lk_subtract_f64_dev(h._h, B * N, _vp(self.d_flux.ptr), _vp(d_model.ptr), _vp(d_corr.ptr),
                                                    _vp(self.stream or None)))
        return self._regress_result(N, K, d_corr, d_outl, d_w, to_host, keep + [d_X, d_cm, d_mu, d_sg, d_model])

    def _regress_result(self, N, K, d_corr, d_outl, d_w, to_host, held):
        """What the three fits return: the host triple ((B, N) arrays on the uniform route, lists per target when ``N`` is None)
        or (corrected batch, d_outl, d_w) with ``held`` kept alive."""
        B, n = len(self), self.n_cadences
        if to_host:
            corrected = d_corr.download(np.float64, n, stream=self.stream)
            outl = d_outl.download(np.uint8, n, stream=self.stream).astype(bool)
            if N is None:
                corrected, outl = np.split(corrected, self.n_off[1:-1]), np.split(outl, self.n_off[1:-1])
            else:
                corrected, outl = corrected.reshape(B, N), outl.reshape(B, N)
            return corrected, outl, d_w.download(np.float64, B * K, stream=self.stream).reshape(B, K)
        out = self._carry(self._new(self.d_time, d_corr, self.d_flux_err, self.n_off, nan_free=self.nan_free, is_sorted=self.is_sorted))
        # scratch and inputs the stream may still be reading: held until the batch is synchronised or dropped
        out._keep = held + [self]
        return out, d_outl, d_w

    # ---------------------------------------------------------------- under-fitting metric, neighbours by index
    def under_fitting_metric(self, neighbors, cadence_mask=None, return_correlations=False, to_host=True, neighbor_batch=None,
                             cadenceno=None, return_common=False):
        """``underfit_metric_neighbors`` (reference correctors/metrics.py:141-257, 451-475) for every target of the batch, the
        neighbours being OTHER TARGETS OF THIS BATCH (the reference fetches them from MAST; after ``cbv_correct`` they are the
        corrected targets of the same field, already in HBM): ``neighbors`` int (B, M), row t = the indices of t's neighbours,
        padded with -1 (``correctors.metrics.nearest_neighbors`` builds it from positions); ``cadence_mask`` bool (N,), shared
        by every target, True = used (the reference's ``lc[cadence_mask]``).  Needs one cadence count for every target and a
        NaN-free batch (``remove_nans()``).  Zero-centred flux is fine (the correlation does not depend on the scale of
        flux / median - 1); a median of exactly zero gives a non-finite result, as in the reference.  Returns metric[B]
        (``to_host=True``; 8 bytes per target cross PCIe) or its ``DeviceBuffer`` (``to_host=False``: nothing synchronised);
        ``return_correlations``: also correlations[B, M] (NaN at padding), host array or ``DeviceBuffer`` likewise.
        ``neighbor_batch``: a resident, NaN-free batch with the same cadence count whose ROWS are the neighbours instead
        (``neighbors`` then holds indices into ``[0, len(neighbor_batch))``, and a target's own row number is a neighbour
        like any other: it names a row of the other batch); its rows are prepared once and only the B targets after them.
        With ``neighbor_batch`` = this batch the result is the same bits as without.

        ``cadenceno``: the strictly increasing integer cadence numbers of the field's grid.  The batch may then be RAGGED
        (``from_fits``, ``remove_nans``, ``remove_outliers``, ``select``) and is matched by its own ``d_cadenceno`` column, as in
        ``regression_correct(cadenceno=)`` (a cadence that is not on the grid is dropped first); ``cadence_mask`` is then ragged:
        bool (sum n,) over the cadences of this batch, or a ``DeviceBuffer`` of that many bytes.  As in the reference, target t
        is compared with its neighbours on the cadences that t (under its mask) and ALL of them have; ``return_common`` adds
        that count, n_common[B] int32, to the result (after the correlations, when both are asked for); fewer than two common
        cadences give NaN, not an error.  A ``neighbor_batch`` is matched to the same grid by its own cadence numbers and its
        rows are not masked (the common cadences are bounded by the target's mask anyway)."""
        what = "under_fitting_metric"
        if cadenceno is None and return_common:
            raise ValueError("under_fitting_metric: return_common goes with cadenceno= (without it every target keeps the same "
                             "cadences)")
        N = self._uniform_n(None, what) if cadenceno is None else None
        if not getattr(self, "nan_free", False):
            raise ValueError("under_fitting_metric needs a NaN-free batch: call remove_nans() first (and cotrend after it)")
        if cadenceno is None:
            layout = _UniformLayout(self, what, N, cadence_mask=cadence_mask)
        else:
            layout = _RowsLayout(self, what, cadenceno, cadence_mask=cadence_mask)
            layout.check_grid()
        layout.check_neighbours(neighbors, neighbor_batch, common=return_common)
        layout.upload()
        cor, B, M = layout.batch, layout.B, layout.M
        d_corr = DeviceBuffer(self.handle, max(B * M, 1) * 8) if return_correlations else None
        d_metric = DeviceBuffer(self.handle, B * 8)
        if neighbor_batch is None:
            layout.under_direct(cor, d_metric, d_corr)
        else:
            layout.neighbour_rows(neighbor_batch)
            layout.under_against(cor, d_metric, 0, d_corr)
        # inputs the stream may still be reading: held until the batch is synchronised or dropped
        self._keep += layout.held()
        out = (d_metric,) + ((d_corr,) if return_correlations else ()) + ((layout.d_nc,) if return_common else ())
        if to_host:
            out = (d_metric.download(np.float64, B, stream=self.stream),)
            if return_correlations:
                out += ((d_corr.download(np.float64, B * M, stream=self.stream) if M else np.empty(0)).reshape(B, M),)
            if return_common:
                out += (layout.d_nc.download(np.int32, B, stream=self.stream),)
        return out if len(out) > 1 else out[0]

    # ---------------------------------------------------------------- over-fitting metric, noise made on the device
    def _overfit_checks(self, original, n_samples, cadence_mask, frequency, seed, first_target, stream_id):
        """Every check of ``over_fitting_metric`` that needs no device -> (N, keep_idx, n, grid or None)."""
        from .device import DeviceLightCurveBatch
        N = self._uniform_n(None, "over_fitting_metric")
        if not isinstance(original, DeviceLightCurveBatch):
            raise ValueError("over_fitting_metric: `original` must be the resident batch before the correction")
        if len(original) != len(self) or original._uniform_n(None, "over_fitting_metric (original)") != N:
            raise ValueError("over_fitting_metric: the original batch must have the targets and cadences of the corrected one "
                             "(%d x %d)" % (len(self), N))
        if not (self.nan_free and original.nan_free):
            raise ValueError("over_fitting_metric needs NaN-free batches: call remove_nans() first (and cotrend after it)")
        if getattr(self, "d_flux_err", None) is None:
            raise ValueError("over_fitting_metric needs the flux errors of the corrected batch (the noise level is their mean)")
        return (N,) + _capi.overfit_arguments(N, n_samples, cadence_mask, frequency, seed, first_target, stream_id, len(self))

    def over_fitting_metric(self, original, frequency=None, n_samples=10, cadence_mask=None, seed=0, first_target=0, stream_id=0,
                            to_host=True, max_scratch_bytes=None):
        """``overfit_metric_lombscargle(original_lc[cadence_mask], corrected_lc[cadence_mask], n_samples)`` (reference
        correctors/metrics.py:24-138, as ``CBVCorrector.over_fitting_metric`` calls it) for every target, called ON THE
        CORRECTED batch; ``original``: the resident batch before the correction (same targets, same cadences).  Both stay in
        HBM: the two periodograms per target, the ``n_samples`` white-noise periodograms and their reduction to one float run
        on the device; 8 bytes per target come back.  ``frequency`` [1/d]: a regular grid shared by the targets; None = the
        grid ``LombScarglePeriodogram.from_lightcurve`` builds (amplitude normalisation, oversample factor 5) for target 0's
        kept cadences (its N times are downloaded once: the targets of a cotrending channel share their cadences; a batch whose
        targets have different times passes ``frequency``).  ``cadence_mask``: bool (N,), True = used.  The noise is not
        ``numpy.random``'s but a counter-based generator's (Philox4x32-10 keyed by ``seed``; counter = (cadence pair, sample,
        ``first_target`` + row, ``stream_id``)): a target's value does not depend on the batch, on ``max_scratch_bytes`` (the
        samples are taken in rounds that keep the scratch block under it; default 4 GiB) or on the run.  Returns metric[B]
        (``to_host=True``) or its ``DeviceBuffer`` (``to_host=False``: nothing synchronised after the periodograms' own
        planning).  Needs one cadence count per batch, NaN-free batches, flux errors on the corrected batch, ``n_samples`` >= 1,
        a regular grid of at least two frequencies and at least three kept cadences: ``ValueError`` before any device call.

        RAGGED batches (``from_fits``, ``remove_nans``, ``remove_outliers``, ``select``; what ``cbv_correct(cadenceno=)`` returns)
        are taken on their own offsets when ``original.n_off`` equals this batch's (``ValueError`` otherwise); ``cadence_mask`` is
        then ragged, bool (sum n,) over the cadences of the batch, or a ``DeviceBuffer`` of that many bytes (downloaded once, to
        list the kept cadences; a ``DeviceBuffer`` is always read as this ragged mask, also on a uniform batch, and for one target the
        two shapes are the same mask); every target needs at least three kept cadences.  A ragged mask also takes a uniform batch this
        way, with the same bits.  ``frequency=None`` stays the grid of target 0's kept times.  Target b's value is the uniform
        call's on a batch that holds its kept cadences alone, with ``first_target + b``."""
        from .device import DeviceLightCurveBatch
        ragged_mask = isinstance(cadence_mask, DeviceBuffer) or (
            cadence_mask is not None and len(self) > 1 and np.shape(cadence_mask) == (self.n_cadences,))
        if isinstance(original, DeviceLightCurveBatch) and (self._is_ragged() or original._is_ragged() or ragged_mask):
            checked = self._overfit_rows_checks(original, n_samples, cadence_mask, frequency, seed, first_target, stream_id)
            layout = _RowsLayout(original, "over_fitting_metric", seed=seed, first_target=first_target, checked=checked)
        else:
            checked = self._overfit_checks(original, n_samples, cadence_mask, frequency, seed, first_target, stream_id)
            layout = _UniformLayout(original, "over_fitting_metric", seed=seed, first_target=first_target, checked=checked)
        metric = layout.over_metric(self, n_samples, stream_id, to_host, max_scratch_bytes)
        self._keep += layout.keep
        return metric

    def _is_ragged(self):
        counts = np.diff(self.n_off)
        return bool(len(counts)) and counts.min() != counts.max()

    def _overfit_rows_checks(self, original, n_samples, cadence_mask, frequency, seed, first_target, stream_id):
        """The checks of the ragged ``over_fitting_metric`` -> (keep_idx or None, k_off, grid or None).  Only a mask given as a
        ``DeviceBuffer`` needs the device (one download), after every check that does not."""
        from .device import DeviceLightCurveBatch
        if not isinstance(original, DeviceLightCurveBatch):
            raise ValueError("over_fitting_metric: `original` must be the resident batch before the correction")
        if len(self) < 1:
            raise ValueError("over_fitting_metric needs at least one light curve")
        if len(original) != len(self) or not np.array_equal(original.n_off, self.n_off):
            rag, name = (self, "corrected") if self._is_ragged() else (original, "original")
            counts = np.diff(rag.n_off)
            raise ValueError("over_fitting_metric: the original batch must have the offsets (n_off) of the corrected one, target by "
                             "target; the %s batch has between %d and %d cadences per target" % (name, counts.min(), counts.max()))
        if not (self.nan_free and original.nan_free):
            raise ValueError("over_fitting_metric needs NaN-free batches: call remove_nans() first (and cotrend after it)")
        if getattr(self, "d_flux_err", None) is None:
            raise ValueError("over_fitting_metric needs the flux errors of the corrected batch (the noise level is their mean)")
        if isinstance(cadence_mask, DeviceBuffer):
            if cadence_mask.nbytes != self.n_cadences:
                raise ValueError("over_fitting_metric: cadence_mask holds %d bytes, the batch has %d cadences"
                                 % (cadence_mask.nbytes, self.n_cadences))
            _capi.overfit_rows_arguments(self.n_off, n_samples, None, frequency, seed, first_target, stream_id)
            cadence_mask = cadence_mask.download(np.uint8, self.n_cadences, stream=self.stream)
        return _capi.overfit_rows_arguments(self.n_off, n_samples, cadence_mask, frequency, seed, first_target, stream_id)

    def cbv_goodness_scan(self, cbvs, alphas, neighbors=None, cbv_indices=np.arange(1, 9), cadence_mask=None, n_samples=1, seed=0,
                          frequency=None, first_target=0, ext_dm=None, sigma=5, niters=5, max_scratch_bytes=None, cadenceno=None):
        """Both goodness metrics of ``cbv_correct`` over a list of ridge penalties, for the whole batch (what
        ``correctors.CBVCorrector.goodness_scan`` does for one target, here for a whole channel): for each
        ``alphas[a]`` the batch is corrected (``cbv_correct(cbvs, cbv_indices, alpha, ext_dm, cadence_mask, sigma, niters)``),
        scored with ``over_fitting_metric(self, ..., stream_id=a)`` and, when ``neighbors`` (int (B, M), see
        ``under_fitting_metric``) is given, with ``under_fitting_metric``.  ``cadence_mask``: bool (N,), shared by the fit and
        both metrics.  A plain loop of resident calls; 8 or 16 bytes per target and penalty come back.  Returns
        dict(alpha[A], over_fitting[A, B], under_fitting[A, B] or None).  ``cadenceno``: the cadence numbers of the rows of
        ``cbvs``; the batch may then be ragged, ``cadence_mask`` is ragged (bool (sum n,) or a ``DeviceBuffer``), and the fit and
        both metrics are ``cbv_correct(cadenceno=)``, the ragged ``over_fitting_metric`` and ``under_fitting_metric(cadenceno=)``:
        the batch is aligned once and the matrix, the mask, the rows and the kept cadences are uploaded once; the result gains
        n_common[A, B] (or None)."""
        alphas = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
        over = dict(n_samples=n_samples, frequency=frequency, seed=seed, first_target=first_target)
        if cadenceno is not None:
            layout = _RowsLayout(self, "cbv_goodness_scan", cadenceno, _cbv_columns(cbvs, cbv_indices, ext_dm), cadence_mask, sigma,
                                 niters, **over)
            out = _goodness_scan(layout, alphas, neighbors, max_scratch_bytes)
            self.synchronize()
            return out
        # (checked as the scan's own calls would: over_fitting_metric's arguments first, then cbv_correct's matrix)
        self._overfit_checks(self, n_samples, cadence_mask, frequency, seed, first_target, 0)
        Xa = _cbv_columns(cbvs, cbv_indices, ext_dm)
        layout = _UniformLayout(self, "cbv_goodness_scan", self._uniform_n(Xa.shape[0], "cbv_correct"), Xa, cadence_mask, sigma, niters,
                                **over)
        return _goodness_scan(layout, alphas, neighbors, max_scratch_bytes)

    def cbv_correct_optimized(self, cbvs, neighbors=None, neighbor_batch=None, cbv_indices=np.arange(1, 9), ext_dm=None,
                              cadence_mask=None, alpha_bounds=(1e-4, 1e4), target_over_score=0.5, target_under_score=0.5,
                              max_iter=100, frequency=None, seed=0, first_target=0, stream_id=0, neighbor_alpha=1e-20, sigma=5,
                              niters=5, max_scratch_bytes=None, return_trace=False, cadenceno=None):
        """``CBVCorrector.correct`` (reference cbvcorrector.py:397-500) for every target of the batch: a bounded Brent search
        of the ridge penalty alpha PER TARGET over ``-(leaky(over, target_over_score) + leaky(under, target_under_score))``
        (``correctors.cbvcorrector.minimize_scalar_bounded`` is the search; every target visits the abscissae that function
        would), one more fit at the optimum, then the over-fitting score with ``n_samples=10`` and the under-fitting score.
        The B searches run in lockstep (``BoundedBrentBatch``): per step 8 bytes per target go up (its alpha) and 16 come back
        (its two scores); a target whose search has ended is evaluated again at its optimum and the value ignored.  The
        design matrix and the mask are uploaded once; what does not depend on alpha is taken once: the periodogram of the
        uncorrected flux, the noise periodogram, the neighbours' normalised rows.  One evaluation is one regression, one
        Lomb-Scargle pass of B rows and one pair pass.

        NOISE: the reference draws fresh noise at every evaluation.  Here the search uses ``n_samples = 1`` and ONE fixed
        stream ``(seed, first_target + b, stream_id)`` for all evaluations (common random numbers): the objective is a
        deterministic function of alpha, and two runs give the same bits.  The final over-fitting score is
        ``over_fitting_metric(n_samples=10)`` with the same seed and stream.

        NEIGHBOURS: rows of the resident ``neighbor_batch`` named by ``neighbors`` (int (B, M), -1 = padding, indices into
        ``[0, len(neighbor_batch))``); their flux is FIXED during the search (``CBVCorrector.set_neighbors``' semantics).
        ``neighbor_batch=None``: this batch corrected at ``neighbor_alpha`` (1e-20: the plain least-squares fit).  A target's
        result therefore depends on its own alpha alone and not on the other targets of the batch.

        A score whose target is <= 0 is skipped (nothing is launched for it): it counts as 1.0 in the objective and is
        reported as -1.0; ``target_under_score > 0`` needs ``neighbors``.  ``cadence_mask``: bool (N,), shared by the fit and
        both metrics; ``frequency``: as in ``over_fitting_metric``.  Returns (corrected ``DeviceLightCurveBatch``, info):
        info = dict(alpha[B], over_fitting_score[B], under_fitting_score[B], objective[B] (the search's best value), nfev[B],
        status[B] (0, or 1 = ``max_iter`` reached)); ``return_trace`` adds trace = dict(alpha[I, B], over[I, B],
        under[I, B]), the I lockstep evaluations (a skipped score is 1.0 there).  Every argument is checked before the first
        device call.

        ``cadenceno``: the cadence numbers of the rows of ``cbvs``.  The batch may then be RAGGED and is matched by its own cadence
        numbers once (``cbv_correct(cadenceno=)``); ``cadence_mask`` is ragged (bool (sum n,) or a ``DeviceBuffer``); the fit, the
        over-fitting session and the under-fitting pair pass run on the batch's own offsets and on the grid
        (``under_fitting_metric(cadenceno=)``: a target meets its neighbours on the cadences it and all of them have); a
        ``neighbor_batch`` is matched to the grid by its own cadence numbers.  The matrix, the mask, the rows and the kept cadences
        are uploaded once; per step still 8 bytes per target go up and 16 come back.  info gains n_common[B] (-1 when the
        under-fitting score is skipped).  A batch in which every target has every grid row gives, without a mask, the bits of the
        call without ``cadenceno`` (under a mask the under-fitting sums run in grid order, not in kept order: equal within
        rounding, the over-fitting scores still bit for bit)."""
        Xa = _cbv_columns(cbvs, cbv_indices, ext_dm)
        what = "cbv_correct_optimized"
        over = dict(n_samples=10, frequency=frequency, seed=seed, first_target=first_target)
        if cadenceno is not None:
            layout = _RowsLayout(self, what, cadenceno, Xa, cadence_mask, sigma, niters, **over)
        else:
            layout = _UniformLayout(self, what, self._uniform_n(Xa.shape[0], what), Xa, cadence_mask, sigma, niters, **over)
        return _ridge_search(layout, neighbors, neighbor_batch, alpha_bounds, target_over_score, target_under_score, max_iter,
                             neighbor_alpha, stream_id, max_scratch_bytes, return_trace)

    def _goodness_rows_setup(self, Nx, cadenceno, cadence_mask, n_samples, frequency, seed, first_target, stream_id, what):
        """The front end the ragged scan and search share: the checks that need no device, ONE alignment, then the kept cadences
        of the aligned batch -> (src, d_rows, d_cm, keep, keep_idx, k_off, d_keep, grid or None)."""
        if not getattr(self, "nan_free", False):
            raise ValueError("%s needs a NaN-free batch: call remove_nans() first" % what)
        if getattr(self, "d_flux_err", None) is None:
            raise ValueError("%s needs flux errors (the ridge width is median(flux_err) / sqrt(|alpha|))" % what)
        if Nx > _capi.UNDERFIT_GRID_MAX_NX:
            raise ValueError("%s: the grid has %d cadences, at most %d are taken" % (what, Nx, _capi.UNDERFIT_GRID_MAX_NX))
        host_mask = None if isinstance(cadence_mask, DeviceBuffer) else cadence_mask
        if host_mask is not None and np.shape(host_mask) != (self.n_cadences,):
            raise ValueError("%s: with `cadenceno` cadence_mask is ragged, one entry per cadence of the batch: shape (%d,) (got %s)"
                             % (what, self.n_cadences, np.shape(host_mask)))
        _capi.overfit_rows_arguments(self.n_off, n_samples, host_mask, frequency, seed, first_target, stream_id)
        src, d_rows, d_cm, keep = self._aligned(Nx, None, cadenceno, cadence_mask, what)
        if d_cm is not None and (host_mask is None or src.n_cadences != self.n_cadences):
            host_mask = d_cm.download(np.uint8, src.n_cadences, stream=self.stream)     # once: it lists the kept cadences
        keep_idx, k_off, grid = _capi.overfit_rows_arguments(src.n_off, n_samples, host_mask, frequency, seed, first_target, stream_id)
        d_keep = None
        if keep_idx is not None:
            d_keep, k = _upload(self.handle, keep_idx, self.stream, np.int32)
            keep.append(k)
        return src, d_rows, d_cm, keep, keep_idx, k_off, d_keep, grid


# ------------------------------------------------------------------------------------------------ what the two layouts share
def _upload_once(layout, on, *items):
    """Every (attribute, host array or None, dtype) that is not in HBM yet goes up on the stream of the batch ``on`` (None: the
    layout's own), the one whose kernels will read it."""
    b = layout.batch if on is None else on
    for name, host, dtype in items:
        if host is not None and getattr(layout, name) is None:
            buf, k = _upload(b.handle, host, b.stream, dtype)
            setattr(layout, name, buf)
            layout.keep.append(k)


def _eval_scores(layout, cor, do_over, do_under, scores):
    """One lockstep evaluation: the scores of ``cor`` into the host ``scores[2, B]`` (row 0 over, row 1 under; a skipped row is
    left as it is).  16 bytes per target come back, 8 when one score is skipped."""
    B = layout.B
    if layout.d_scores is None:
        layout.d_scores = DeviceBuffer(cor.handle, 2 * B * 8)
    if do_over:
        layout.session_eval(cor, layout.d_scores)
    if do_under:
        layout.under_against(cor, layout.d_scores, B * 8)
    if do_over and do_under:
        layout.d_scores.download(np.float64, 2 * B, out=scores.reshape(-1), stream=cor.stream)
    elif do_over or do_under:
        layout.d_scores.download(np.float64, B, out=scores[0 if do_over else 1], stream=cor.stream, offset_bytes=0 if do_over else B * 8)


def _final_under(layout, cor):
    """The under-fitting score of ``cor`` against the prepared rows -> float64[B] on the host."""
    d_under = DeviceBuffer(cor.handle, layout.B * 8)
    layout.under_against(cor, d_under, 0)
    return d_under.download(np.float64, layout.B, stream=cor.stream)


# ------------------------------------------------------------------------------------------------ the two layouts
class _UniformLayout(object):
    """A batch with ONE cadence count ``N``: row j of the design matrix ``Xa`` is cadence j of every target, ``cadence_mask`` is
    bool (N,) and shared.  Holds what a scan or a search uploads once and calls the uniform C entry points.  ``batch``: the
    batch that is fitted (for the over-fitting metric: the one before the correction); ``cor``: a corrected batch to score."""

    eval_scores, final_under = _eval_scores, _final_under       # (the same code on both layouts)

    def __init__(self, batch, what, N=None, Xa=None, cadence_mask=None, sigma=5, niters=5, n_samples=10, frequency=None, seed=0,
                 first_target=0, checked=None):
        self.batch, self.what, self.N, self.Xa, self.cadence_mask, self.sigma, self.niters = (
            batch, what, N, Xa, cadence_mask, sigma, niters)
        self.n_samples, self.frequency, self.seed, self.first_target = n_samples, frequency, seed, first_target
        self.B, self.flux_errors = len(batch), getattr(batch, "d_flux_err", None) is not None
        self.n, self.keep_idx, self.grid, self.nb, self.Bn, self.M = N, None, None, None, None, 0
        self.d_X = self.d_cm = self.d_keep = self.d_nb = self.d_rows = self.d_sess = self.d_scores = None
        self.nbr_flux, self.keep = None, []
        if checked is not None:         # one over_fitting_metric call: what its ``_overfit_checks`` returned, nothing to prepare
            self.N, self.keep_idx, self.n, self.grid = checked

    # ---- the checks that need no device
    def check_neighbours(self, neighbors, neighbor_batch, fixed=False, common=False):
        """``fixed``: the neighbours are rows prepared once (a search), so a target's own number is a row like any other."""
        self.Bn = (self.B if fixed else None) if neighbor_batch is None else _check_neighbor_batch(neighbor_batch, self.what, self.N)
        self.nb, self.keep_idx, self.n = _capi.underfit_arguments(self.B, self.N, neighbors, self.cadence_mask, self.Bn)
        self.M = self.nb.shape[1]

    def prepare(self, neighbors, neighbor_batch, stream_id, fixed):
        """Every check of a scan or a search that this layout owns, then the uploads."""
        b = self.batch
        self.N, self.keep_idx, self.n, self.grid = b._overfit_checks(b, self.n_samples, self.cadence_mask, self.frequency, self.seed,
                                                                     self.first_target, stream_id)
        if neighbors is not None:
            self.check_neighbours(neighbors, neighbor_batch, fixed)
        self.upload()

    def upload(self, on=None):
        """Resident once: X, the fit's mask, the kept cadences, the neighbour table, queued on the stream of ``on`` (the batch
        whose kernels read them; default: the layout's own)."""
        fit_mask = None
        if self.Xa is not None and self.cadence_mask is not None and self.d_cm is None:
            fit_mask = np.ascontiguousarray(np.broadcast_to(np.asarray(self.cadence_mask, dtype=bool), (self.B, self.N)), dtype=np.uint8)
        _upload_once(self, on, ("d_X", self.Xa, np.float64), ("d_cm", fit_mask, np.uint8), ("d_keep", self.keep_idx, np.int32),
                     ("d_nb", self.nb if self.M else None, np.int32))

    # ---- the fit
    def fit(self, alphas=None, alpha=None):
        b, held = self.batch, []
        d_mu, d_sg = b._ridge_prior(self.N, self.Xa.shape[1], alpha, alphas, held)
        return b._regress_shared(self.Xa, self.N, d_mu, d_sg, None, self.sigma, self.niters, False, held, resident=(self.d_X, self.d_cm))[0]

    # ---- the over-fitting metric
    def default_grid(self, cor=None):
        """The default frequency grid of target 0's kept times (its times are downloaded once)."""
        b = self.batch if cor is None else cor
        t0 = b.d_time.download(np.float64, self.N, stream=b.stream)
        return _capi.overfit_default_grid(t0 if self.keep_idx is None else t0[self.keep_idx])

    def over_metric(self, cor, n_samples, stream_id, to_host, max_scratch_bytes):
        h, B, st = cor.handle, self.B, _vp(cor.stream or None)
        if self.grid is None:
            self.grid = _capi.overfit_grid(self.default_grid(cor))
        f0, df, nf = self.grid
        nbytes, _rounds = _capi.overfit_scratch_bytes(B, self.n, nf, n_samples, max_scratch_bytes)
        self.upload(cor)
        # (the scratch block goes back to the free list when this call returns: work on one handle is stream-ordered)
        d_scr, d_metric = DeviceBuffer(h, nbytes), DeviceBuffer(h, B * 8)
        _capi._check(_capi._lib.lk_overfit_metric_batch_dev(
            h._h, B, self.N, _vp(cor.d_time.ptr), _vp(self.batch.d_flux.ptr), _vp(cor.d_flux.ptr), _vp(cor.d_flux_err.ptr), self.n,
            _p(self.d_keep), f0, df, nf, int(n_samples), int(self.seed), int(self.first_target), int(stream_id), _vp(d_scr.ptr),
            nbytes, _vp(d_metric.ptr), st))
        cor._keep += [self.d_keep, self.batch]
        return d_metric.download(np.float64, B, stream=cor.stream) if to_host else d_metric

    def session_begin(self, stream_id, max_scratch_bytes):
        b = self.batch
        if self.grid is None:
            self.grid = _capi.overfit_grid(self.default_grid())
        f0, df, nf = self.grid
        self.sess_bytes = _capi.overfit_scratch_bytes(self.B, self.n, nf, 1, max_scratch_bytes)[0]
        self.d_sess = DeviceBuffer(b.handle, self.sess_bytes)
        _capi._check(_capi._lib.lk_overfit_session_begin_dev(
            b.handle._h, self.B, self.N, _vp(b.d_time.ptr), _vp(b.d_flux.ptr), self.n, _p(self.d_keep), f0, df, nf, 1, int(self.seed),
            int(self.first_target), int(stream_id), _vp(self.d_sess.ptr), self.sess_bytes, _vp(b.stream or None)))

    def session_eval(self, cor, d_scores):
        f0, df, nf = self.grid
        _capi._check(_capi._lib.lk_overfit_session_eval_dev(
            cor.handle._h, self.B, self.N, _vp(cor.d_flux.ptr), _vp(cor.d_flux_err.ptr), self.n, _p(self.d_keep), f0, df, nf, 1,
            _vp(self.d_sess.ptr), self.sess_bytes, _vp(d_scores.ptr), _vp(cor.stream or None)))

    # ---- the under-fitting metric
    def under_direct(self, cor, d_metric, d_corr=None):
        """Against the batch's own targets."""
        _capi._check(_capi._lib.lk_underfit_neighbors_batch_dev(
            cor.handle._h, self.B, self.N, _vp(cor.d_flux.ptr), self.n, _p(self.d_keep), self.M, _p(self.d_nb),
            _p(d_corr if self.M else None), _vp(d_metric.ptr), _vp(cor.stream or None)))

    def neighbour_rows(self, neighbor_batch, neighbor_alpha=None):
        """The neighbours' rows, prepared once (queued on the stream of the batch that will read them).  ``neighbor_batch=None``:
        this batch corrected at ``neighbor_alpha``."""
        if neighbor_batch is None:
            neighbor_batch = self.fit(alpha=neighbor_alpha)
        h, Bn = neighbor_batch.handle, len(neighbor_batch)
        nbytes = ctypes.c_int64(0)
        _capi._check(_capi._lib.lk_underfit_rows_bytes(Bn, self.n, ctypes.byref(nbytes)))
        self.d_rows = DeviceBuffer(h, nbytes.value)
        _capi._check(_capi._lib.lk_underfit_rows_prepare_dev(h._h, Bn, self.N, _vp(neighbor_batch.d_flux.ptr), self.n, _p(self.d_keep),
                                                             _vp(self.d_rows.ptr), nbytes.value, _vp(self.batch.stream or None)))
        # (the neighbours' flux buffer, not the batch: a batch that holds a batch can close a reference cycle — with itself as
        # its own neighbour batch it would — and a cycle's buffers come back only when the cyclic collector runs)
        self.nbr_flux, self.Bn = neighbor_batch.d_flux, Bn

    def under_against(self, cor, d_metric, offset, d_corr=None):
        """The pair pass of ``cor``'s targets against the prepared rows, into ``d_metric`` ``offset`` bytes in."""
        _capi._check(_capi._lib.lk_underfit_against_rows_batch_dev(
            cor.handle._h, self.B, self.N, _vp(cor.d_flux.ptr), self.n, _p(self.d_keep), self.Bn, _vp(self.d_rows.ptr), self.M,
            _p(self.d_nb), _p(d_corr if self.M else None), _p(d_metric, offset), _vp(cor.stream or None)))

    def held(self):
        """What must outlive the stream's work: into the ``_keep`` of the batch that is handed out."""
        return self.keep + [self.d_keep, self.d_nb, self.d_rows, self.nbr_flux]

    def extra_info(self, do_under, scan=False):
        return {}


class _RowsLayout(object):
    """A batch on its own offsets (it may be ragged) whose cadences name rows of the design matrix ``Xa`` / of the grid
    ``cadenceno``; ``cadence_mask`` is ragged (bool (sum n,) or a ``DeviceBuffer``).  The same operations as ``_UniformLayout`` on
    the rows C entry points.  ``batch`` becomes the ALIGNED batch once ``upload`` / ``prepare`` has matched it to the grid."""

    eval_scores, final_under = _eval_scores, _final_under       # (the same code on both layouts)

    def __init__(self, batch, what, cadenceno=None, Xa=None, cadence_mask=None, sigma=5, niters=5, n_samples=10, frequency=None, seed=0,
                 first_target=0, checked=None):
        self.batch, self.what, self.cadenceno, self.Xa, self.cadence_mask, self.sigma, self.niters = (
            batch, what, cadenceno, Xa, cadence_mask, sigma, niters)
        self.n_samples, self.frequency, self.seed, self.first_target = n_samples, frequency, seed, first_target
        self.B, self.flux_errors = len(batch), getattr(batch, "d_flux_err", None) is not None
        self.Nx = Xa.shape[0] if Xa is not None else (None if cadenceno is None else int(np.asarray(cadenceno).size))
        self.keep_idx, self.k_off, self.grid, self.nb, self.Bn, self.M = None, batch.n_off, None, None, None, 0
        self.d_X = self.d_cm = self.d_keep = self.d_nb = self.d_rows = self.d_block = self.d_sess = self.d_scores = self.d_nc = None
        self.common, self.keep = False, []
        if checked is not None:         # one over_fitting_metric call: what its ``_overfit_rows_checks`` returned, no grid to match
            self.keep_idx, self.k_off, self.grid = checked

    # ---- the checks that need no device
    def check_grid(self):
        if self.Nx > _capi.UNDERFIT_GRID_MAX_NX:
            raise ValueError("%s: the grid has %d cadences, at most %d are taken" % (self.what, self.Nx, _capi.UNDERFIT_GRID_MAX_NX))

    def check_neighbours(self, neighbors, neighbor_batch, fixed=False, common=True):
        """``fixed``: the neighbours are rows prepared once (a search), so a target's own number is a row like any other.
        ``common``: the pair passes also count the common cadences (``upload`` makes room for them)."""
        self.common = common
        self.Bn = (self.B if fixed else None) if neighbor_batch is None else _check_neighbor_batch(neighbor_batch, self.what)
        self.nb = _capi.underfit_arguments(self.B, max(self.Nx, 2), neighbors, None, self.Bn)[0]
        self.M = self.nb.shape[1]

    def prepare(self, neighbors, neighbor_batch, stream_id, fixed):
        """Every check of a scan or a search that this layout owns, ONE alignment, then the uploads."""
        if neighbors is not None:
            self.check_neighbours(neighbors, neighbor_batch, fixed)
        self.batch, self.d_rows, self.d_cm, self.keep, self.keep_idx, self.k_off, self.d_keep, self.grid = self.batch._goodness_rows_setup(
            self.Nx, self.cadenceno, self.cadence_mask, self.n_samples, self.frequency, self.seed, self.first_target, stream_id, self.what)
        self.upload()

    def upload(self, on=None):
        """Resident once: the alignment (unless ``prepare`` made it), X, the kept cadences, the neighbour table and room for the
        common-cadence counts, queued on the stream of ``on`` (the batch whose kernels read them; default: the layout's own)."""
        if self.d_rows is None and self.cadenceno is not None:
            self.batch, self.d_rows, self.d_cm, self.keep = self.batch._aligned(self.Nx, None, self.cadenceno, self.cadence_mask, self.what)
        _upload_once(self, on, ("d_X", self.Xa, np.float64), ("d_keep", self.keep_idx, np.int32),
                     ("d_nb", self.nb if self.M else None, np.int32))
        if self.common and self.d_nc is None:
            self.d_nc = DeviceBuffer(self.batch.handle, self.B * 4)

    # ---- the fit
    def fit(self, alphas=None, alpha=None):
        b, held = self.batch, []
        d_mu, d_sg = b._ridge_prior(None, self.Xa.shape[1], alpha, alphas, held)
        return b._regress_shared_rows(self.Xa, self.d_rows, d_mu, d_sg, self.d_cm, self.sigma, self.niters, False, held,
                                      resident=self.d_X)[0]

    # ---- the over-fitting metric
    def _p_koff(self):
        return _off_ptr(self.k_off) if self.keep_idx is not None else None

    def default_grid(self, cor=None):
        """The default frequency grid of target 0's kept times (its times are downloaded once)."""
        b = self.batch if cor is None else cor
        t0 = b.d_time.download(np.float64, int(b.n_off[1]), stream=b.stream)
        return _capi.overfit_default_grid(t0 if self.keep_idx is None else t0[self.keep_idx[:int(self.k_off[1])]])

    def over_metric(self, cor, n_samples, stream_id, to_host, max_scratch_bytes):
        h, B, st = cor.handle, self.B, _vp(cor.stream or None)
        if self.grid is None:
            self.grid = _capi.overfit_grid(self.default_grid(cor))
        f0, df, nf = self.grid
        nbytes, _rounds = _capi.overfit_scratch_rows_bytes(self.k_off, nf, n_samples, max_scratch_bytes)
        self.upload(cor)
        d_scr, d_metric = DeviceBuffer(h, nbytes), DeviceBuffer(h, B * 8)
        _capi._check(_capi._lib.lk_overfit_metric_rows_batch_dev(
            h._h, B, _off_ptr(cor.n_off), _vp(cor.d_time.ptr), _vp(self.batch.d_flux.ptr), _vp(cor.d_flux.ptr), _vp(cor.d_flux_err.ptr),
            _p(self.d_keep), self._p_koff(), f0, df, nf, int(n_samples), int(self.seed), int(self.first_target), int(stream_id),
            _vp(d_scr.ptr), nbytes, _vp(d_metric.ptr), st))
        cor._keep += [self.d_keep, self.batch.d_flux]
        return d_metric.download(np.float64, B, stream=cor.stream) if to_host else d_metric

    def session_begin(self, stream_id, max_scratch_bytes):
        b = self.batch
        if self.grid is None:
            self.grid = _capi.overfit_grid(self.default_grid())
        f0, df, nf = self.grid
        self.sess_bytes = _capi.overfit_scratch_rows_bytes(self.k_off, nf, 1, max_scratch_bytes)[0]
        self.d_sess = DeviceBuffer(b.handle, self.sess_bytes)
        _capi._check(_capi._lib.lk_overfit_session_begin_rows_dev(
            b.handle._h, self.B, _off_ptr(b.n_off), _vp(b.d_time.ptr), _vp(b.d_flux.ptr), _p(self.d_keep), self._p_koff(), f0, df, nf, 1,
            int(self.seed), int(self.first_target), int(stream_id), _vp(self.d_sess.ptr), self.sess_bytes, _vp(b.stream or None)))

    def session_eval(self, cor, d_scores):
        f0, df, nf = self.grid
        _capi._check(_capi._lib.lk_overfit_session_eval_rows_dev(
            cor.handle._h, self.B, _off_ptr(self.batch.n_off), _vp(cor.d_flux.ptr), _vp(cor.d_flux_err.ptr), _p(self.d_keep),
            self._p_koff(), f0, df, nf, 1, _vp(self.d_sess.ptr), self.sess_bytes, _vp(d_scores.ptr), _vp(cor.stream or None)))

    # ---- the under-fitting metric
    def under_direct(self, cor, d_metric, d_corr=None):
        """Against the batch's own targets, on the grid."""
        _capi._check(_capi._lib.lk_underfit_grid_neighbors_batch_dev(
            cor.handle._h, self.B, _off_ptr(cor.n_off), _vp(self.d_rows.ptr), self.Nx, _vp(cor.d_flux.ptr), _p(self.d_cm), self.M,
            _p(self.d_nb), _p(d_corr if self.M else None), _p(self.d_nc), _vp(d_metric.ptr), _vp(cor.stream or None)))

    def _grid_block(self, batch, d_rows, d_cm):
        """The light curves of an aligned ``batch`` prepared as grid neighbour rows -> their ``DeviceBuffer``."""
        nbytes = ctypes.c_int64(0)
        _capi._check(_capi._lib.lk_underfit_grid_rows_bytes(len(batch), self.Nx, ctypes.byref(nbytes)))
        d_block = DeviceBuffer(batch.handle, nbytes.value)
        _capi._check(_capi._lib.lk_underfit_grid_rows_prepare_dev(
            batch.handle._h, len(batch), _off_ptr(batch.n_off), _vp(d_rows.ptr), self.Nx, _vp(batch.d_flux.ptr), _p(d_cm),
            _vp(d_block.ptr), nbytes.value, _vp(self.batch.stream or None)))
        return d_block

    def neighbour_rows(self, neighbor_batch, neighbor_alpha=None):
        """The neighbours' rows on the grid, prepared once.  ``neighbor_batch=None``: this batch corrected at ``neighbor_alpha``
        (the same cadences, so the same rows and the same mask); a ``neighbor_batch`` is matched to the grid by its own cadence
        numbers and is not masked."""
        if neighbor_batch is None:
            nbr = self.fit(None, neighbor_alpha)
            self.d_block = self._grid_block(nbr, self.d_rows, self.d_cm)
            self.keep += [nbr.d_flux]
        else:
            src, d_rows, _, keep = neighbor_batch._aligned(self.Nx, None, self.cadenceno, None, "under_fitting_metric (neighbor_batch)")
            self.d_block, self.Bn = self._grid_block(src, d_rows, None), len(src)
            self.keep += keep + [d_rows, src.d_flux]

    def under_against(self, cor, d_metric, offset, d_corr=None):
        """The grid pair pass of ``cor``'s targets against the prepared rows, into ``d_metric`` ``offset`` bytes in."""
        _capi._check(_capi._lib.lk_underfit_grid_against_rows_batch_dev(
            cor.handle._h, self.B, _off_ptr(cor.n_off), _vp(self.d_rows.ptr), self.Nx, _vp(cor.d_flux.ptr), _p(self.d_cm), self.Bn,
            _vp(self.d_block.ptr), self.M, _p(self.d_nb), _p(d_corr if self.M else None), _p(self.d_nc), _p(d_metric, offset),
            _vp(cor.stream or None)))

    def held(self):
        """What must outlive the stream's work: into the ``_keep`` of the batch that is handed out (the flux buffer, not the
        aligned batch: see ``_UniformLayout.neighbour_rows``)."""
        b = self.batch
        return self.keep + [self.d_X, self.d_rows, self.d_cm, self.d_keep, self.d_nb, self.d_block, self.d_sess, b.d_flux, b.d_time]

    def extra_info(self, do_under, scan=False):
        """n_common[B] of the last pair pass; skipped: None in a scan, -1 in a search."""
        if not do_under:
            return dict(n_common=None if scan else np.full(self.B, -1, dtype=np.int32))
        return dict(n_common=self.d_nc.download(np.int32, self.B, stream=self.batch.stream))


# ------------------------------------------------------------------------------------------------ the scan and the search
def _goodness_scan(layout, alphas, neighbors, max_scratch_bytes):
    """``cbv_goodness_scan`` on either layout: fit, over-fitting metric (stream a) and direct pair pass per penalty."""
    layout.prepare(neighbors, None, 0, False)
    if layout.grid is None:      # the default grid depends on the times alone: taken once for the whole scan
        layout.grid = _capi.overfit_grid(layout.default_grid())
    B, stream, do_under = layout.B, layout.batch.stream, neighbors is not None
    over = np.empty((len(alphas), B))
    under = np.empty((len(alphas), B)) if do_under else None
    extra = layout.extra_info(False, scan=True)          # n_common on the rows layout: None until there are neighbours
    if do_under:
        extra = {key: np.empty((len(alphas), B), dtype=np.int32) for key in extra}
    d_under = DeviceBuffer(layout.batch.handle, B * 8) if do_under else None
    for a, alpha in enumerate(alphas):
        cor = layout.fit(alpha=float(alpha))
        d_over = layout.over_metric(cor, layout.n_samples, a, False, max_scratch_bytes)
        if do_under:
            layout.under_direct(cor, d_under)
        over[a] = d_over.download(np.float64, B, stream=stream)
        if do_under:
            under[a] = d_under.download(np.float64, B, stream=stream)
            for key, row in layout.extra_info(True).items():
                extra[key][a] = row
        cor.synchronize()
    return dict(alpha=alphas, over_fitting=over, under_fitting=under, **extra)


def _ridge_search(layout, neighbors, neighbor_batch, alpha_bounds, target_over_score, target_under_score, max_iter, neighbor_alpha,
                  stream_id, max_scratch_bytes, return_trace):
    """``cbv_correct_optimized`` on either layout (``layout.B`` targets).  Everything that touches the device is the layout's: this
    function holds the argument checks, the lockstep Brent search over the leaky objective, the trace, the fit at the optimum
    with its final scores, and ``info``."""
    from .correctors.cbvcorrector import BoundedBrentBatch
    lo, hi = float(alpha_bounds[0]), float(alpha_bounds[1])
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo > hi:
        raise ValueError("alpha_bounds must be two finite penalties, lower first (got %r)" % (tuple(alpha_bounds),))
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1 (got %r)" % (max_iter,))
    t_over, t_under = float(target_over_score), float(target_under_score)
    do_over, do_under = t_over > 0, t_under > 0
    if do_under and neighbors is None:
        raise ValueError("target_under_score > 0 needs `neighbors` (and `neighbor_batch`, or this batch's own targets corrected "
                         "at neighbor_alpha): pass target_under_score=0 to search on the over-fitting metric alone")
    if not np.isfinite(float(neighbor_alpha)):
        raise ValueError("neighbor_alpha must be finite (got %r)" % (neighbor_alpha,))
    if not layout.flux_errors:
        raise ValueError("cbv_correct_optimized needs flux errors (the ridge width is median(flux_err) / sqrt(|alpha|))")
    # ---- resident once: X, the masks, the over-fitting session, the neighbour rows
    layout.prepare(neighbors if do_under else None, neighbor_batch, stream_id, True)
    if do_over:
        layout.session_begin(stream_id, max_scratch_bytes)
    if do_under:
        layout.neighbour_rows(neighbor_batch, float(neighbor_alpha))
    # ---- the lockstep search
    B = layout.B
    brent = BoundedBrentBatch((lo, hi), B, maxiter=int(max_iter))
    scores = np.ones((2, B))
    trace = dict(alpha=[], over=[], under=[])
    while not brent.done.all():
        alphas = brent.x.copy()
        cor = layout.fit(alphas)
        layout.eval_scores(cor, do_over, do_under, scores)
        cor.synchronize()
        brent.tell(-(_leaky_scores(scores[0], t_over) + _leaky_scores(scores[1], t_under)))
        if return_trace:
            trace["alpha"].append(alphas), trace["over"].append(scores[0].copy()), trace["under"].append(scores[1].copy())
    res = brent.result()
    # ---- the fit at the optimum and its scores
    out = layout.fit(res["x"])
    over, under = np.full(B, -1.0), np.full(B, -1.0)
    if do_over:
        over = layout.over_metric(out, 10, stream_id, True, max_scratch_bytes)
    if do_under:
        under = layout.final_under(out)
    info = dict(alpha=res["x"], over_fitting_score=over, under_fitting_score=under, objective=res["fun"], nfev=res["nfev"],
                status=res["status"])
    info.update(layout.extra_info(do_under))
    out._keep += layout.held()
    if return_trace:
        info["trace"] = {k: np.array(v, dtype=np.float64).reshape(len(v), B) for k, v in trace.items()}
    return out, info


class _RaggedMask(object):
    """A ragged ``cadence_mask`` (bool (sum n,) on the host, or a ``DeviceBuffer`` of that many bytes) of ``batch``, checked when
    made.  ``route``: how the message names what makes the mask ragged.  A ``DeviceBuffer`` is used as it is unless cadences
    are dropped: then it is downloaded once and the kept part goes up again."""

    def __init__(self, batch, cadence_mask, route, what):
        n = batch.n_cadences
        self.batch, self.host, self.dev = batch, None, None
        if isinstance(cadence_mask, DeviceBuffer):
            if cadence_mask.nbytes != n:
                raise ValueError("%s: cadence_mask holds %d bytes, the batch has %d cadences" % (what, cadence_mask.nbytes, n))
            self.dev = cadence_mask
        elif cadence_mask is not None:
            self.host = np.ascontiguousarray(cadence_mask, dtype=np.uint8)
            if self.host.shape != (n,):
                raise ValueError("%s: %s cadence_mask is ragged, one entry per cadence of the batch: shape (%d,) (got %s)"
                                 % (what, route, n, self.host.shape))

    def drop(self, gone):
        """Without the cadences where ``gone`` (bool over the batch's cadences) is true."""
        b = self.batch
        if self.dev is not None:
            self.host, self.dev = self.dev.download(np.uint8, b.n_cadences, stream=b.stream), None
        if self.host is not None:
            self.host = np.ascontiguousarray(self.host[~gone])

    def on_device(self, keep):
        """The mask's ``DeviceBuffer`` (a host mask is uploaded, its staging appended to ``keep``), or None."""
        if self.host is None:
            return self.dev
        d_cm, k = _upload(self.batch.handle, self.host, self.batch.stream, np.uint8)
        keep.append(k)
        return d_cm


def _design_arrays(X, prior_mu, prior_sigma):
    """(X float64 (N, K), prior_mu, prior_sigma) of a shared design matrix: a host array, a ``DesignMatrix`` or a
    ``DesignMatrixCollection`` (whose own priors stand in when none are given)."""
    if hasattr(X, "prior_sigma") and hasattr(X, "X"):
        if prior_mu is None and prior_sigma is None:
            prior_mu, prior_sigma = np.asarray(X.prior_mu, dtype=np.float64), np.asarray(X.prior_sigma, dtype=np.float64)
        X = X.X
    Xa = np.ascontiguousarray(X, dtype=np.float64)
    if Xa.ndim != 2 or Xa.shape[1] < 1:
        raise ValueError("the design matrix must be 2-D (cadences x regressors), got shape %s" % (Xa.shape,))
    if (prior_mu is None) != (prior_sigma is None):
        raise ValueError("Please specify both `prior_mu` and `prior_sigma`")
    if prior_mu is not None:
        prior_mu, prior_sigma = np.asarray(prior_mu, dtype=np.float64), np.asarray(prior_sigma, dtype=np.float64)
    return Xa, prior_mu, prior_sigma


def _cadenceno_array(a, n, name):
    """Integer cadence numbers / row indices -> int32 (n,), C-contiguous; ``ValueError`` for another shape, kind or range."""
    a = np.asarray(a)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must be an integer array of shape (%d,) (got %s of shape %s)" % (name, n, a.dtype, a.shape))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("%s must fit int32" % name)
    return np.ascontiguousarray(a, dtype=np.int32)


def _alpha_per_target(alpha, B):
    """One ridge penalty per target -> float64[B]; ``ValueError`` unless B finite, non-zero values."""
    a = np.ascontiguousarray(alpha, dtype=np.float64)
    if a.shape != (B,):
        raise ValueError("alpha must be a scalar or one penalty per target, shape (%d,) (got shape %s)" % (B, a.shape))
    if not np.all(np.isfinite(a)) or np.any(a == 0.0):
        raise ValueError("every alpha of an array must be finite and non-zero (no prior is the scalar alpha == 0.0)")
    return a


def _leaky_scores(metric, target, leak=0.01):
    """``correctors.cbvcorrector._leaky`` on an array of scores: above the target a score counts with 1 % of its excess."""
    if target > 0:
        return np.where(metric >= target, target + leak * (metric - target), metric)
    return metric


def _check_neighbor_batch(neighbor_batch, what, N=None):
    """The checks of a ``neighbor_batch`` that need no device -> its number of rows.  ``N``: it must have that one cadence count
    (the uniform layout); None: it must carry cadence numbers (the rows layout matches it to the grid by them)."""
    from .device import DeviceLightCurveBatch
    if not isinstance(neighbor_batch, DeviceLightCurveBatch):
        raise ValueError("%s: `neighbor_batch` must be a resident DeviceLightCurveBatch" % what)
    if N is not None:
        Nn = neighbor_batch._uniform_n(None, "%s (neighbor_batch)" % what)
        if Nn != N:
            raise ValueError("%s: neighbor_batch has %d cadences per target, this batch has %d" % (what, Nn, N))
    if not getattr(neighbor_batch, "nan_free", False):
        raise ValueError("%s needs a NaN-free neighbor_batch: call remove_nans() first (and cotrend after it)" % what)
    if N is None and getattr(neighbor_batch, "d_cadenceno", None) is None:
        raise ValueError("%s(cadenceno=) needs a neighbor_batch that carries cadence numbers" % what)
    return len(neighbor_batch)


def _cbv_columns(cbvs, cbv_indices, ext_dm):
    """The columns ``CBVCorrector._collection`` builds — [cbvs[:, idx - 1] | ext_dm | 1] — as one float64 (N, K) array."""
    from .correctors.cbvcorrector import cbv_index_list
    cbvs = np.asarray(cbvs, dtype=np.float64)
    if cbvs.ndim != 2:
        raise ValueError("cbvs must be 2-D (cadences x vectors)")
    mats = []
    if cbv_indices is not None:
        mats.append(cbvs[:, cbv_index_list(cbv_indices, cbvs.shape[1]) - 1])
    if ext_dm is not None:
        if not (hasattr(ext_dm, "X") and hasattr(ext_dm, "prior_sigma")):
            raise ValueError("ext_dm must be a DesignMatrix")
        if ext_dm.shape[0] != cbvs.shape[0]:
            raise ValueError("ext_dm must contain the same number of cadences as the basis vectors")
        mats.append(np.asarray(ext_dm.X, dtype=np.float64))
    if not mats:
        raise ValueError("nothing to fit: pass cbv_indices and/or ext_dm")
    mats.append(np.ones((cbvs.shape[0], 1)))
    return np.ascontiguousarray(np.hstack(mats))
