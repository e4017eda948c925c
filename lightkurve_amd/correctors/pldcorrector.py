"""PLDCorrector over the GPU design-matrix + regression path
(reference: src/lightkurve/correctors/pldcorrector.py:109-120, 125-287, 304-427).

The reference takes a ``TargetPixelFile``; that container (FITS I/O, WCS, plotting) is out of scope, so the mirror
takes a ``PixelCube``: time[N], flux[N, ny, nx], flux_err[N, ny, nx] and an optional mission string — the only
things ``PLDCorrector`` reads from the TPF — with the two TPF helpers it calls
(``create_threshold_mask`` targetpixelfile.py:680-742, aperture photometry :868-923)."""
import logging

import numpy as np

from .. import _capi
from ..lightcurve import LightCurve
from .designmatrix import (DesignMatrix, DesignMatrixCollection, SparseDesignMatrixCollection,
                           create_sparse_spline_matrix)
from .regressioncorrector import RegressionCorrector

log = logging.getLogger(__name__)

__all__ = ["PixelCube", "PLDCorrector", "pld_correct_batch", "threshold_mask_from_median_image", "centroid_quadratic"]

# (A^T A)^-1 A^T of the 3 x 3 quadratic fit P = a + b x + c y + d x^2 + e x y + f y^2, x fastest, x, y in {0, 1, 2}: these
# integers over 36, exactly (the table csrc/pixcube.hip carries)
_QUADRATIC_FIT_36 = np.array([[29, 8, -1, 8, -4, -4, -1, -4, 5], [-27, 24, 3, -18, 24, -6, -9, 24, -15],
                              [-27, -18, -9, 24, 24, 24, 3, -6, -15], [6, -12, 6, 6, -12, 6, 6, -12, 6],
                              [9, 0, -9, 0, 0, 0, -9, 0, 9], [6, 6, 6, -12, -12, -12, 6, 6, 6]], dtype=np.float64)


def centroid_quadratic(data, mask=None, return_peak=False):
    """``lightkurve.utils.centroid_quadratic``: the extremum of the quadratic fitted to the 3 x 3 patch around the brightest
    pixel of ``data * mask`` -> (column, row) in pixel indices (a symmetric source centred on pixel (i, j) gives (i, j)).  The
    patch is clamped into the image; a NaN inside it, a flat patch (``|det| < 1e-6``) or an image without any value gives
    (nan, nan) — the reference raises on the last.  ``return_peak`` adds the flat index of the brightest pixel (before the
    clamp; -1 without one).  The host mirror of ``lk_cube_centroids_quadratic_batch_dev``."""
    z = np.asarray(data, dtype=np.float64)
    if z.ndim != 2 or z.shape[0] < 3 or z.shape[1] < 3:
        raise ValueError("centroid_quadratic needs an image of at least 3 x 3 pixels (got shape {})".format(z.shape))
    with np.errstate(all="ignore"):
        if mask is not None:
            mask = np.asarray(mask, dtype=bool)
            if mask.shape != z.shape:
                raise ValueError("`mask` has shape {}, but the image has shape {}".format(mask.shape, z.shape))
            z = z * mask
        col = row = np.nan
        valid = ~np.isnan(z)
        if not valid.any():
            return (col, row, -1) if return_peak else (col, row)
        k = int(np.argmax(np.where(valid, z, -np.inf)))
        if np.isnan(z.flat[k]):                      # (every value is -inf: argmax may sit on a NaN before the first of them)
            k = int(np.flatnonzero(valid.ravel())[0])
        ny, nx = z.shape
        yy, xx = min(max(k // nx, 1), ny - 2), min(max(k % nx, 1), nx - 2)
        a, b, c, d, e, f = _QUADRATIC_FIT_36.dot(z[yy - 1:yy + 2, xx - 1:xx + 2].ravel()) / 36.0
        det = 4 * d * f - e ** 2
        if not abs(det) < 1e-6:
            col = xx - 1 + (-(2 * f * b - c * e) / det)
            row = yy - 1 + (-(2 * d * c - b * e) / det)
    return (float(col), float(row), k) if return_peak else (float(col), float(row))


def _moment_centroids(flux, ap, column=0, row=0):
    """The moment centroids of the images flux[..., ny, nx] inside the boolean aperture ``ap`` -> (col, row): float64 nansums,
    a zero or NaN total gives NaN."""
    yy, xx = np.indices(ap.shape)
    with np.errstate(all="ignore"):
        f = np.where(ap, np.asarray(flux, dtype=np.float64), np.nan)
        tot = np.nansum(f, axis=(-2, -1))
        tot = np.where(tot == 0, np.nan, tot)
        return np.nansum((column + xx) * f, axis=(-2, -1)) / tot, np.nansum((row + yy) * f, axis=(-2, -1)) / tot


def _transit_classes(time, period, transit_time, duration, in_width=0.5, out_inner=1.0, out_outer=2.0):
    """uint8 per cadence: 1 in transit (``|x| < in_width * duration``), 2 out of transit (``out_inner * duration <= |x| <
    out_outer * duration``), 0 otherwise and for a NaN time; x = the phase of ``create_transit_mask``."""
    if not (0 < in_width <= out_inner < out_outer):
        raise ValueError("need 0 < in_width <= out_inner < out_outer (got %r, %r, %r)" % (in_width, out_inner, out_outer))
    period, transit_time, duration = float(period), float(transit_time), float(duration)
    if not (period != 0 and np.isfinite(period) and np.isfinite(transit_time) and np.isfinite(duration)):
        raise ValueError("period, transit_time and duration must be finite and the period non-zero")
    with np.errstate(all="ignore"):
        hp = period / 2.0
        x = np.abs(np.mod(np.asarray(time, dtype=np.float64) - transit_time + hp, period) - hp)
        cls = np.zeros(x.shape, dtype=np.uint8)
        cls[x < in_width * duration] = 1
        cls[(x >= out_inner * duration) & (x < out_outer * duration)] = 2
    return cls


def threshold_mask_from_median_image(median_image, threshold=3, reference_pixel="center"):
    """The second half of ``create_threshold_mask`` (targetpixelfile.py:700-742): the MAD cut and the 4-connected labelling on
    the per-pixel nanmedian image (row, column) — shared with ``DevicePixelCubeBatch``, which computes that image on the GPU."""
    median_image = np.asarray(median_image, dtype=np.float64)
    if reference_pixel == "center":
        reference_pixel = (median_image.shape[1] / 2, median_image.shape[0] / 2)
    with np.errstate(all="ignore"):
        vals = median_image[np.isfinite(median_image)].flatten()
        mad = np.median(np.abs(vals - np.median(vals)))
        mad_cut = (1.4826 * mad * threshold) + np.nanmedian(median_image)
        mask = np.nan_to_num(median_image) >= mad_cut
    if reference_pixel is None or not mask.any():
        return mask
    labels = np.zeros(mask.shape, dtype=int)
    current = 0
    for r in range(mask.shape[0]):
        for c in range(mask.shape[1]):
            if mask[r, c] and labels[r, c] == 0:
                current += 1
                labels[r, c] = current
                stack = [(r, c)]
                while stack:
                    a, b = stack.pop()
                    for da, db in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                        aa, bb = a + da, b + db
                        if (0 <= aa < mask.shape[0] and 0 <= bb < mask.shape[1] and mask[aa, bb]
                                and labels[aa, bb] == 0):
                            labels[aa, bb] = current
                            stack.append((aa, bb))
    args = np.argwhere(labels > 0)
    dist = [np.hypot(a[0] - reference_pixel[1], a[1] - reference_pixel[0]) for a in args]
    closest = args[int(np.argmin(dist))]
    return labels == labels[closest[0], closest[1]]


def _background_meta(npix, bkg):
    """The meta keys a background subtraction leaves: ``npix`` mask pixels (-1: unknown), ``bkg`` the subtracted [N] values."""
    return {"BKG_SUBTRACTED": True, "BKG_NPIX": int(npix), "BKG_NAN_CADENCES": int(np.sum(np.isnan(bkg)))}


def _psf_sigma(sigma):
    """``sigma`` of ``psf_photometry``: a scalar or (sigma_col, sigma_row) -> the pair, finite and > 0."""
    sg = np.asarray(sigma, dtype=np.float64)
    if sg.shape not in ((), (2,)):
        raise ValueError("sigma must be a scalar or (sigma_col, sigma_row) (got shape %r)" % (sg.shape,))
    sg = np.broadcast_to(sg, (2,))
    if not (np.all(np.isfinite(sg)) and np.all(sg > 0)):
        raise ValueError("sigma must be finite and > 0 (got %r)" % (sigma,))
    return float(sg[0]), float(sg[1])


def _psf_fit_parameters(max_iter, tol, max_step, max_shift):
    """The iteration's parameters of ``psf_fit``, checked: max_iter an integer 1 .. 64, tol finite and >= 0, max_step and
    max_shift > 0."""
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= 64:
        raise ValueError("max_iter must be an integer 1 .. 64 (got %r)" % (max_iter,))
    tol, max_step, max_shift = float(tol), float(max_step), float(max_shift)
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("tol must be finite and >= 0 (got %r)" % (tol,))
    if not (max_step > 0 and max_shift > 0):
        raise ValueError("max_step and max_shift must be > 0 (got %r and %r)" % (max_step, max_shift))
    return int(max_iter), tol, max_step, max_shift


def _psf_width_parameters(max_iter, tol, max_step, min_sigma, max_sigma, sigma0):
    """The iteration's parameters of ``psf_width``, checked: max_iter an integer 1 .. 64, tol finite and >= 0, max_step > 0,
    0 < min_sigma <= sigma0 <= max_sigma with both bounds finite; ``sigma0``: (sigma_col, sigma_row) or [B, 2]."""
    max_iter, tol, _, _ = _psf_fit_parameters(max_iter, tol, 1.0, 1.0)
    max_step, min_sigma, max_sigma = float(max_step), float(min_sigma), float(max_sigma)
    if not max_step > 0:
        raise ValueError("max_step must be > 0 (got %r)" % (max_step,))
    if not (np.isfinite(min_sigma) and np.isfinite(max_sigma) and min_sigma > 0):
        raise ValueError("min_sigma and max_sigma must be finite, min_sigma > 0 (got %r and %r)" % (min_sigma, max_sigma))
    s0 = np.asarray(sigma0, dtype=np.float64)
    if not (np.all(s0 >= min_sigma) and np.all(s0 <= max_sigma)):
        raise ValueError("need min_sigma <= sigma0 <= max_sigma (got %r, %r, %r)" % (min_sigma, sigma0, max_sigma))
    return max_iter, tol, max_step, min_sigma, max_sigma


def _psf_width_tables(c, sg, n):
    """The n pixel factors of ``psf_width`` along one axis at the centres ``c`` (any shape) and the width ``sg``, and their
    derivatives by ``sg`` -> two arrays c.shape + (n,): (erf(z_{k+1}) - erf(z_k)) / 2 and -(Q(k + 1) - Q(k)), z_k = (k - 1/2 - c) /
    (sqrt(2) sg), Q(k) = (k - 1/2 - c) exp(-z_k^2) / (sqrt(2 pi) sg^2)."""
    import math
    x = np.arange(n + 1) - 0.5 - np.asarray(c, dtype=np.float64)[..., None]
    z = x / (np.sqrt(2.0) * sg)
    E, Q = np.vectorize(math.erf, otypes=[np.float64])(z), x * np.exp(-z * z) / (np.sqrt(2.0 * np.pi) * sg * sg)
    return 0.5 * (E[..., 1:] - E[..., :-1]), -(Q[..., 1:] - Q[..., :-1])


def _psf_positions_parameters(max_iter, tol, max_step, max_offset):
    """The iteration's parameters of ``psf_positions``, checked: max_iter an integer 1 .. 64, tol finite and >= 0, max_step > 0,
    max_offset > 0."""
    max_iter, tol, _, _ = _psf_fit_parameters(max_iter, tol, 1.0, 1.0)
    max_step, max_offset = float(max_step), float(max_offset)
    if not max_step > 0:
        raise ValueError("max_step must be > 0 (got %r)" % (max_step,))
    if not max_offset > 0:
        raise ValueError("max_offset must be > 0 (got %r)" % (max_offset,))
    return max_iter, tol, max_step, max_offset


def _psf_centre_tables(c, sg, n):
    """The n pixel factors of the PSF calls along one axis at the centres ``c`` (any shape) and the width ``sg``, and their
    derivatives by the centre -> two arrays c.shape + (n,): (erf(z_{k+1}) - erf(z_k)) / 2 and -(P(k + 1) - P(k)), z_k = (k - 1/2
    - c) / (sqrt(2) sg), P(k) = exp(-z_k^2) / (sqrt(2 pi) sg): the tables of ``psf_fit``, where a shift and a centre enter as
    one sum."""
    import math
    z = (np.arange(n + 1) - 0.5 - np.asarray(c, dtype=np.float64)[..., None]) / (np.sqrt(2.0) * sg)
    E, P = np.vectorize(math.erf, otypes=[np.float64])(z), np.exp(-z * z) / (np.sqrt(2.0 * np.pi) * sg)
    return 0.5 * (E[..., 1:] - E[..., :-1]), -(P[..., 1:] - P[..., :-1])


def _psf_cholesky(G, scale):
    """The unpivoted Cholesky of the PSF fits: G (M, k, k), pivot cut 1e-12 scale (M, k) -> L, singular, smallest pivot ratio."""
    M, k = G.shape[:2]
    L, singular, ratio = np.zeros((M, k, k)), np.zeros(M, dtype=bool), np.full(M, np.inf)
    for q in range(k):
        d = G[:, q, q].copy()
        for j in range(q):
            d -= L[:, q, j] * L[:, q, j]
        singular |= ~(np.isfinite(d) & (d > 1e-12 * scale[:, q]))
        ratio = np.minimum(ratio, np.where(np.isfinite(d) & (scale[:, q] > 0), d / scale[:, q], 0.0))
        L[:, q, q] = np.sqrt(d)
        for i in range(q + 1, k):
            s_ = G[:, q, i].copy()
            for j in range(q):
                s_ -= L[:, i, j] * L[:, q, j]
            L[:, i, q] = s_ / L[:, q, q]
    return L, singular, ratio


def _psf_forward(L, B):
    """L^-1 B, B (M, k, m)."""
    Y = np.zeros_like(B)
    for i in range(L.shape[1]):
        s_ = B[:, i].copy()
        for j in range(i):
            s_ -= L[:, i, j, None] * Y[:, j]
        Y[:, i] = s_ / L[:, i, i, None]
    return Y


def _psf_backward(L, Y):
    """L^-T Y."""
    X = np.zeros_like(Y)
    for i in range(L.shape[1] - 1, -1, -1):
        s_ = Y[:, i].copy()
        for j in range(i + 1, L.shape[1]):
            s_ -= L[:, j, i, None] * X[:, j]
        X[:, i] = s_ / L[:, i, i, None]
    return X


class TabulatedPRF(object):
    """A tabulated, pixel-integrated PRF and its interpolation — the model of ``psf_photometry(prf=)``, plain numpy, and the
    definition of what ``lk_cube_prf_photometry_batch_dev`` evaluates on the device.  ``samples``: [Ty, Tx] or [n_prf, Ty, Tx],
    kept as float32 (as the mission files are); every value finite; Ty, Tx >= 1, no parity requirement.  ``oversample``: an
    integer os >= 1.  Sample (j, i) is the fraction of a star's flux collected by a pixel whose centre lies ((i - (Tx - 1) / 2) /
    os, (j - (Ty - 1) / 2) / os) px from the star's centre.  Nothing is normalised.  The value at an offset (dx, dy) is Keys' cubic
    convolution (a = -1/2, Catmull-Rom) on the table continued by zeros, all in float64: u = dx os + (Tx - 1) / 2, i0 = floor(u),
    f = u - i0 (likewise v, j0, g), w_-1 = ((-f + 2) f - 1) f / 2, w_0 = ((3 f - 5) f f + 2) / 2, w_1 = ((-3 f + 4) f + 1) f / 2,
    w_2 = (f - 1) f f / 2, P = sum_jj w_jj(g) (sum_ii w_ii(f) T[j0 + jj][i0 + ii]), ii and jj from -1 to 2 in that order, T = 0
    outside the table.  os is an integer, so the pixels of an image share f and g: i0 and f are formed ONCE per axis, at pixel 0
    (dx = 0 - col), and pixel ix reads the taps i0 + ix os + ii.  A centre with |u| >= 1e9 or NaN has no tap on the table (f = 0).
    No file is read and the five corner tables of a channel are not blended: the caller passes the blended array."""

    FAR = 1e9

    def __init__(self, samples, oversample):
        s = np.asarray(samples)
        if s.ndim == 2:
            s = s[None]
        if s.ndim != 3 or min(s.shape) < 1:
            raise ValueError("samples must be [Ty, Tx] or [n_prf, Ty, Tx] with every size >= 1 (got shape %r)" % (np.shape(samples),))
        with np.errstate(all="ignore"):
            s = np.array(s, dtype=np.float32, order="C")
        if not np.all(np.isfinite(s)):
            raise ValueError("every sample of a PRF table must be finite (as float32)")
        if isinstance(oversample, bool) or int(oversample) != oversample or int(oversample) < 1:
            raise ValueError("oversample must be an integer >= 1 (got %r)" % (oversample,))
        s.setflags(write=False)
        self.samples, self.oversample = s, int(oversample)

    @property
    def n_prf(self):
        return self.samples.shape[0]

    @classmethod
    def from_gaussian(cls, sigma_col, sigma_row, oversample, half_width):
        """The pixel-integrated Gaussian of ``psf_photometry(sigma=)`` sampled on a table that reaches ``half_width`` px to every
        side of the centre: 2 round(half_width os) + 1 samples per axis."""
        import math
        sig_c, sig_r = _psf_sigma((sigma_col, sigma_row))
        os_ = int(oversample)
        if os_ != oversample or os_ < 1 or not half_width * os_ >= 0.5:
            raise ValueError("need an integer oversample >= 1 and half_width * oversample >= 1/2")
        d = np.arange(-int(round(half_width * os_)), int(round(half_width * os_)) + 1) / float(os_)
        erf = np.vectorize(math.erf, otypes=[np.float64])
        gx = 0.5 * (erf((d + 0.5) / (np.sqrt(2.0) * sig_c)) - erf((d - 0.5) / (np.sqrt(2.0) * sig_c)))
        gy = 0.5 * (erf((d + 0.5) / (np.sqrt(2.0) * sig_r)) - erf((d - 0.5) / (np.sqrt(2.0) * sig_r)))
        return cls(gy[:, None] * gx[None, :], os_)

    def _check_index(self, index):
        if isinstance(index, (bool, np.bool_)) or np.ndim(index) != 0 or int(index) != index or not 0 <= int(index) < self.n_prf:
            raise ValueError("prf_index must be an integer 0 .. %d (got %r)" % (self.n_prf - 1, index))
        return int(index)

    def _axis(self, c, n, size):
        """One axis: centres ``c`` (any shape, px from the centre of pixel 0), ``n`` pixels, ``size`` samples -> the table
        indices c.shape + (n, 4) of the four taps of every pixel (``size`` = the zero beyond the table) and the weights
        c.shape + (4,)."""
        os_ = self.oversample
        u = (0.0 - np.asarray(c, dtype=np.float64)) * os_ + 0.5 * (size - 1)
        far = ~(np.abs(u) < self.FAR)
        fl = np.floor(np.where(far, 0.0, u))
        f = np.where(far, 0.0, u - fl)
        w = np.stack([((-f + 2.0) * f - 1.0) * f * 0.5, ((3.0 * f - 5.0) * f * f + 2.0) * 0.5,
                      ((-3.0 * f + 4.0) * f + 1.0) * f * 0.5, (f - 1.0) * f * f * 0.5], axis=-1)
        idx = fl.astype(np.int64)[..., None, None] - 1 + np.arange(4) + (np.arange(n) * os_)[:, None]
        return np.where(far[..., None, None] | (idx < 0) | (idx >= size), size, idx), w

    def evaluate(self, shape, col, row, index=0):
        """The model image(s) of a star of unit flux centred (``col``, ``row``) px from the centre of pixel (0, 0) of a (ny, nx)
        image: float64 of shape broadcast(col, row).shape + (ny, nx)."""
        ny, nx = (int(v) for v in shape)
        _, Ty, Tx = self.samples.shape
        T = np.zeros((Ty + 1, Tx + 1))
        T[:Ty, :Tx] = self.samples[self._check_index(index)]
        col, row = np.broadcast_arrays(np.asarray(col, dtype=np.float64), np.asarray(row, dtype=np.float64))
        with np.errstate(all="ignore"):
            jx, wx = self._axis(col, nx, Tx)
            jy, wy = self._axis(row, ny, Ty)
            acc = np.zeros(col.shape + (ny, nx))
            for jj in range(4):
                r = np.zeros(col.shape + (ny, nx))
                for ii in range(4):
                    r = r + wx[..., None, None, ii] * T[jy[..., :, None, jj], jx[..., None, :, ii]]
                acc = acc + wy[..., None, None, jj] * r
        return acc

    def evaluate_with_gradient(self, shape, col, row, index=0):
        """``evaluate`` and its derivatives by the star's centre -> (P, dP/dcol, dP/drow), each of ``evaluate``'s shape; P has
        ``evaluate``'s bits.  The gradients use the same taps with the derivative weights of the same f: w'_-1 = ((-3 f + 4) f -
        1) / 2, w'_0 = (9 f - 10) f / 2, w'_1 = ((-9 f + 8) f + 1) / 2, w'_2 = (3 f - 2) f / 2, each multiplied by du/dc = -os
        (u = (0 - c) os + (T - 1) / 2 falls as the centre rises): dP/dcol = sum_jj w_jj(g) (sum_ii w'_ii(f) T), dP/drow = sum_jj
        w'_jj(g) (sum_ii w_ii(f) T), in ``evaluate``'s order.  Keys' interpolant is C1, so the gradients are continuous; a far or
        NaN centre gives zero for all three.  The model of ``psf_fit(prf=)``."""
        ny, nx = (int(v) for v in shape)
        _, Ty, Tx = self.samples.shape
        T = np.zeros((Ty + 1, Tx + 1))
        T[:Ty, :Tx] = self.samples[self._check_index(index)]
        col, row = np.broadcast_arrays(np.asarray(col, dtype=np.float64), np.asarray(row, dtype=np.float64))
        with np.errstate(all="ignore"):
            jx, wx = self._axis(col, nx, Tx)
            jy, wy = self._axis(row, ny, Ty)
            dx, dy = self._axis_derivative(col, Tx), self._axis_derivative(row, Ty)
            acc, acc_c, acc_r = (np.zeros(col.shape + (ny, nx)) for _ in range(3))
            for jj in range(4):
                r, rc = np.zeros(col.shape + (ny, nx)), np.zeros(col.shape + (ny, nx))
                for ii in range(4):
                    t = T[jy[..., :, None, jj], jx[..., None, :, ii]]
                    r = r + wx[..., None, None, ii] * t
                    rc = rc + dx[..., None, None, ii] * t
                acc = acc + wy[..., None, None, jj] * r
                acc_c = acc_c + wy[..., None, None, jj] * rc
                acc_r = acc_r + dy[..., None, None, jj] * r
        return acc, acc_c, acc_r

    def _axis_derivative(self, c, size):
        """One axis: the derivatives of ``_axis``'s weights by the centre c, c.shape + (4,): w'(f) x (-os); zeros for a far
        centre."""
        os_ = self.oversample
        u = (0.0 - np.asarray(c, dtype=np.float64)) * os_ + 0.5 * (size - 1)
        far = ~(np.abs(u) < self.FAR)
        f = np.where(far, 0.0, u - np.floor(np.where(far, 0.0, u)))
        d = np.stack([((-3.0 * f + 4.0) * f - 1.0) * 0.5, (9.0 * f - 10.0) * f * 0.5, ((-9.0 * f + 8.0) * f + 1.0) * 0.5,
                      (3.0 * f - 2.0) * f * 0.5], axis=-1) * (-float(os_))
        return np.where(far[..., None], 0.0, d)


class PixelCube(object):
    """Minimal stand-in for the slice of TargetPixelFile that PLDCorrector touches."""

    def __init__(self, time, flux, flux_err, mission=None, targetid=None):
        self.time = np.asarray(time, dtype=np.float64)
        self.flux = np.asarray(flux)
        self.flux_err = np.asarray(flux_err)
        if self.flux.ndim != 3 or self.flux.shape != self.flux_err.shape or len(self.time) != len(self.flux):
            raise ValueError("flux and flux_err must be (cadence, row, column) cubes matching time")
        self.meta = {"MISSION": mission, "TARGETID": targetid}

    @classmethod
    def from_fits(cls, path, quality_bitmask="default", device=0):
        """A Kepler / K2 / TESS target-pixel file -> the arrays PLDCorrector works on, with the reference's cadence
        selection (``KeplerTargetPixelFile`` / ``TessTargetPixelFile``: targetpixelfile.py:2120-2122, 2794-2801).  Headers
        are parsed on the host (fitsio.py), the table's bytes are turned into time / quality / float32 cubes on the GPU
        (``lk_fits_unpack_cube``).  Also sets ``flux_bkg`` (when the file has it), ``quality`` and ``pipeline_mask``
        (aperture extension & 2, targetpixelfile.py:308-322)."""
        from .. import _capi, fitsio
        tab = fitsio.read_fits_table(path, ext=1)
        pc = fitsio.pixel_columns(tab, quality_bitmask=quality_bitmask)
        t, q, cubes = _capi.fits_unpack_cube(tab.raw, pc["off_time"], pc["code_time"], pc["off_quality"], pc["code_quality"],
                                             pc["bitmask"], pc["keep_nan_time"], pc["col_offsets"], pc["npix"], device=device)
        shape = (len(t),) + tuple(pc["shape"])
        by_name = {n: cubes[i].reshape(shape) for i, n in enumerate(pc["columns"])}
        flux = by_name["flux"]
        err = by_name.get("flux_err", np.full(shape, np.nan, dtype=np.float32))
        mission = tab.primary.get("MISSION", tab.primary.get("TELESCOP"))
        out = cls(t, flux, err, mission=mission, targetid=tab.primary.get("KEPLERID", tab.primary.get("TICID")))
        out.quality = q
        out.flux_bkg = by_name.get("flux_bkg")
        aper = fitsio.read_fits_image(path, 2)
        out.pipeline_mask = (aper & 2) > 0 if aper is not None and aper.shape == shape[1:] else np.ones(shape[1:], dtype=bool)
        out.meta.update({"FILENAME": str(path), "QUALITY_BITMASK": quality_bitmask, "LABEL": tab.primary.get("OBJECT")})
        return out

    @property
    def shape(self):
        return self.flux.shape

    def __getitem__(self, key):
        c = PixelCube(self.time[key], self.flux[key], self.flux_err[key])
        c.meta = dict(self.meta)
        return c

    def create_threshold_mask(self, threshold=3, reference_pixel="center"):
        """Pixels whose median flux exceeds median + threshold * 1.4826 * MAD; with a reference pixel, only the
        4-connected region closest to it (targetpixelfile.py:680-742)."""
        with np.errstate(all="ignore"):
            median_image = np.nanmedian(np.asarray(self.flux, dtype=np.float64), axis=0)
        return threshold_mask_from_median_image(median_image, threshold, reference_pixel)

    def _parse_aperture_mask(self, aperture_mask):
        """'all' / None, 'threshold', 'background' (= not threshold), 'empty', or a boolean (row, column) array
        (targetpixelfile.py:603-678; 'pipeline' needs the FITS aperture extension and is not available here)."""
        if aperture_mask is None or (isinstance(aperture_mask, str) and aperture_mask == "all"):
            return np.ones(self.shape[1:], dtype=bool)
        if isinstance(aperture_mask, str):
            if aperture_mask == "threshold":
                return self.create_threshold_mask()
            if aperture_mask == "background":
                return ~self.create_threshold_mask(threshold=0, reference_pixel=None)
            if aperture_mask == "empty":
                return np.zeros(self.shape[1:], dtype=bool)
            raise ValueError("aperture_mask '{}' is not supported here".format(aperture_mask))
        m = np.asarray(aperture_mask, dtype=bool)
        if m.shape != self.shape[1:]:
            raise ValueError("`aperture_mask` has shape {}, but the flux data has shape {}".format(m.shape,
                                                                                                 self.shape[1:]))
        return m

    def to_lightcurve(self, aperture_mask=None):
        """Simple aperture photometry, flux_method='sum' (targetpixelfile.py:868-923); numpy keeps float32 cubes
        float32 here exactly like the reference does."""
        flux, flux_err = self._aperture_sums(self._parse_aperture_mask(aperture_mask))
        lc = LightCurve(time=self.time, flux=flux, flux_err=flux_err, meta=dict(self.meta))
        lc._flux_f32 = np.asarray(flux, dtype=np.float32)   # the value the reference carries (float32 for FITS cubes)
        return lc

    def estimate_centroids(self, aperture_mask="all", method="moments", column=0, row=0):
        """``TargetPixelFile.estimate_centroids(aperture_mask, method)`` -> (col[N], row[N]) float64, ``column`` / ``row`` = the
        cutout's corner.  'moments': the flux-weighted mean pixel position inside the aperture (nansum; a zero or NaN total
        gives NaN).  'quadratic': ``centroid_quadratic`` of every cadence (NaN where the reference would raise).  The host
        mirror of ``DevicePixelCubeBatch.estimate_centroids``."""
        ap = self._parse_aperture_mask(aperture_mask)
        if method == "moments":
            return _moment_centroids(self.flux, ap, column, row)
        if method != "quadratic":
            raise ValueError("method must be 'moments' or 'quadratic' (got {!r})".format(method))
        cr = np.array([centroid_quadratic(im, ap) for im in self.flux], dtype=np.float64).reshape(-1, 2)
        return column + cr[:, 0], row + cr[:, 1]

    def estimate_background(self, aperture_mask="background", return_scatter=False):
        """``TargetPixelFile.estimate_background(aperture_mask)``: the per-pixel background of every cadence as the median of
        the pixels in ``aperture_mask`` (default 'background', the complement of ``create_threshold_mask(0, None)``, made from
        the cube as it is).  The host mirror of ``DevicePixelCubeBatch.estimate_background``, and its definition.  With ``sel =
        flux[:, mask]`` in float32 (pixels in ascending flat index), a dict of ``flux`` float32[N] = ``np.nanmedian(sel,
        axis=1)`` (NaN is the only excluded value, +-inf are values; an even count gives float32(a + b) / 2; no value, or an empty
        mask, gives NaN and no warning), ``n_pixels`` int32[N] = the values of ``sel`` that are not NaN, ``mask`` bool (ny, nx) and,
        with ``return_scatter``, ``scatter`` float32[N] = ``np.nanmedian(|sel - flux[:, None]|, axis=1)`` in float32.  No error
        column: the reference's estimate has none."""
        import warnings
        m = self._parse_aperture_mask(aperture_mask)
        sel = np.asarray(self.flux, dtype=np.float32)[:, m]

        def nanmedian_rows(a):
            if a.shape[1] == 0:
                return np.full(a.shape[0], np.nan, dtype=np.float32)
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore", RuntimeWarning)
                return np.asarray(np.nanmedian(a, axis=1), dtype=np.float32)

        out = {"flux": nanmedian_rows(sel), "n_pixels": np.sum(~np.isnan(sel), axis=1).astype(np.int32), "mask": m}
        if return_scatter:
            with np.errstate(all="ignore"):
                out["scatter"] = nanmedian_rows(np.abs(sel - out["flux"][:, None]))
        return out

    def subtract_background(self, background=None, aperture_mask="background"):
        """A new ``PixelCube`` with ``flux - bkg[:, None, None]`` in float32.  ``bkg``: ``estimate_background(aperture_mask)
        ["flux"]`` when ``background`` is None, else the given float32-castable [N] array or the dict ``estimate_background``
        returned.  ``flux_err`` and ``time`` are carried unchanged (the estimate has no error).  ``meta`` gains ``BKG_SUBTRACTED``
        = True, ``BKG_NPIX`` = the pixels of the mask (-1 for a bare array) and ``BKG_NAN_CADENCES`` = the cadences whose
        background is NaN.  The host mirror of ``DevicePixelCubeBatch.subtract_background``."""
        if background is None:
            background = self.estimate_background(aperture_mask)
        npix = -1
        if isinstance(background, dict):
            npix = int(np.sum(background["mask"]))
            background = background["flux"]
        bkg = np.asarray(background, dtype=np.float32)
        if bkg.shape != (len(self.time),):
            raise ValueError("background must hold one value per cadence (%d), got shape %r" % (len(self.time), bkg.shape))
        with np.errstate(all="ignore"):
            flux = np.asarray(self.flux, dtype=np.float32) - bkg[:, None, None]
        out = PixelCube(self.time, flux, self.flux_err)
        out.meta = dict(self.meta)
        out.meta.update(_background_meta(npix, bkg))
        return out

    def difference_image(self, period, transit_time, duration, in_width=0.5, out_inner=1.0, out_outer=2.0,
                         aperture_mask="all", column=0, row=0):
        """The transit difference image of this cutout and where it sits (the host mirror of
        ``DevicePixelCubeBatch.difference_images``, in numpy; same keys without the batch axis).  Cadences are classed by the
        phase of ``create_transit_mask``: in transit where ``|x| < in_width * duration``, out of transit where ``out_inner *
        duration <= |x| < out_outer * duration``.  ``mean_in`` / ``mean_out``: per-pixel nanmean over each class; ``diff`` =
        mean_out - mean_in (positive where the dimming is); ``diff_err`` from ``flux_err`` over the same values.
        ``centroid_diff`` / ``centroid_out`` (quadratic) and ``..._moments``: (col, row) inside ``aperture_mask``; ``offset`` =
        centroid_diff - centroid_out, ``offset_pix`` its norm.  ``status``: 0 ok, 1 no in-transit cadence, 2 no out-of-transit
        cadence, 3 centroid undefined."""
        ap = self._parse_aperture_mask(aperture_mask)
        cls = _transit_classes(self.time, period, transit_time, duration, in_width, out_inner, out_outer)
        flux = np.asarray(self.flux, dtype=np.float64)
        err2 = np.asarray(self.flux_err, dtype=np.float64) ** 2
        out = {"cadence_class": cls, "n_in": int(np.sum(cls == 1)), "n_out": int(np.sum(cls == 2))}
        with np.errstate(all="ignore"):
            part = {}
            for name, sel in (("in", cls == 1), ("out", cls == 2)):
                f = flux[sel]
                ok = ~np.isnan(f)
                n = ok.sum(axis=0).astype(np.float64)
                part[name] = (np.where(ok, f, 0.0).sum(axis=0) / n, np.where(ok, err2[sel], 0.0).sum(axis=0) / (n * n))
            out["mean_in"], out["mean_out"] = part["in"][0], part["out"][0]
            out["diff"] = out["mean_out"] - out["mean_in"]
            out["diff_err"] = np.sqrt(part["in"][1] + part["out"][1])
        for key, im in (("diff", out["diff"]), ("out", out["mean_out"])):
            c, r = centroid_quadratic(im, ap)
            out["centroid_" + key] = np.array([column + c, row + r])
            out["centroid_%s_moments" % key] = np.array([v[0] for v in _moment_centroids(im[None], ap, column, row)])
        out["offset"] = out["centroid_diff"] - out["centroid_out"]
        out["offset_pix"] = float(np.sqrt(np.sum(out["offset"] ** 2)))
        out["status"] = 1 if out["n_in"] == 0 else 2 if out["n_out"] == 0 else 3 if np.isnan(out["offset_pix"]) else 0
        return out

    def amplitude_image(self, frequency, nterms=1, aperture_mask="all", column=0, row=0):
        """The amplitude image of this cutout at one ``frequency`` [1/d] and where it sits: the periodic twin of
        ``difference_image`` (the host mirror of ``DevicePixelCubeBatch.amplitude_images``, in float64 numpy after the float32
        load; same keys without the batch axis).  ``t_ref`` is the first finite time; cadences with a non-finite time are
        dropped and pixel p is fitted, unweighted, on the cadences where its own flux is not NaN (``n_used[p]`` of them) by the
        design of ``ls_model_host(t[ok], y[ok, p], None, frequency, nterms, singular="nan")``: columns [1, sin(2 pi m f (t -
        t_ref)), cos(2 pi m f (t - t_ref))], m = 1 .. ``nterms`` (1 .. 3), K = 2 nterms + 1, y centred on its mean.
        ``theta`` (K, ny, nx): the bias, then sin 1, cos 1, ...; ``level`` = y_mean + bias, the mean image under the signal;
        ``amplitude`` (nterms, ny, nx) = hypot(s_m, c_m); ``phase`` = atan2(c_m, s_m), of A sin(w (t - t_ref) + phase);
        ``chi2`` = sum (y - model)^2; with sigma2 = chi2 / (n_used - K) and C the inverse of the pixel's normal matrix,
        ``amplitude_err`` = sqrt(sigma2 (s^2 C_ss + 2 s c C_sc + c^2 C_cc)) / amplitude and ``snr`` = amplitude /
        amplitude_err.  A pixel with n_used < K or a singular or non-finite fit is NaN in every float image, one with n_used
        == K has NaN ``amplitude_err`` and ``snr``; nothing is raised per pixel.  ``centroid_amp`` / ``centroid_level``
        (quadratic) and ``..._moments``: (col, row) of ``amplitude[0]`` and ``level`` inside ``aperture_mask``; ``offset`` =
        centroid_amp - centroid_level, ``offset_pix`` its norm.  ``status``: 0 ok; 1 the frequency is NaN or <= 0, 2 fewer than
        K + 1 cadences with a finite time (the cutout is skipped: NaN images, ``n_used`` 0); 3 a quadratic centroid is NaN."""
        if int(nterms) != nterms or not 1 <= int(nterms) <= 3:
            raise ValueError("nterms must be an integer 1 .. 3 (got %r)" % (nterms,))
        if np.ndim(frequency) != 0:
            raise ValueError("frequency must be one number per cutout (got shape %r)" % (np.shape(frequency),))
        ny, nx = self.shape[1:]
        if ny < 3 or nx < 3:
            raise ValueError("the quadratic centroid needs cutouts of at least 3 x 3 pixels (got %d x %d)" % (ny, nx))
        ap = self._parse_aperture_mask(aperture_mask)
        nterms, f = int(nterms), float(frequency)
        K = 2 * nterms + 1
        fin = np.isfinite(self.time)
        t_ref = float(self.time[fin][0]) if fin.any() else np.nan
        status = 1 if not (f > 0 and np.isfinite(f)) else 2 if fin.sum() < K + 1 else 0
        out = {"frequency": f, "t_ref": t_ref, "theta": np.full((K, ny, nx), np.nan), "n_used": np.zeros((ny, nx), dtype=np.int32)}
        for key in ("level", "chi2"):
            out[key] = np.full((ny, nx), np.nan)
        for key in ("amplitude", "phase", "amplitude_err", "snr"):
            out[key] = np.full((nterms, ny, nx), np.nan)
        if status == 0:
            t = self.time[fin] - t_ref
            y = np.asarray(self.flux, dtype=np.float64)[fin].reshape(len(t), ny * nx)
            cols = [np.ones(len(t))]
            for m in range(1, nterms + 1):
                cols += [np.sin(2 * np.pi * m * f * t), np.cos(2 * np.pi * m * f * t)]
            X_all = np.column_stack(cols)
            with np.errstate(all="ignore"):
                for p in range(ny * nx):
                    iy, ix = divmod(p, nx)
                    ok = ~np.isnan(y[:, p])
                    n = int(ok.sum())
                    out["n_used"][iy, ix] = n
                    if n < K:
                        continue
                    X, yp = (X_all, y[:, p]) if n == len(t) else (X_all[ok], y[ok, p])
                    y_mean = yp.sum() / n
                    G = X.T.dot(X)
                    try:
                        sol = np.linalg.solve(G, X.T.dot(yp - y_mean))
                        C = np.linalg.inv(G)
                    except np.linalg.LinAlgError:
                        continue
                    level = y_mean + sol[0]
                    if not (np.all(np.isfinite(sol)) and np.isfinite(level)):
                        continue
                    chi2 = float(np.sum((yp - (y_mean + X.dot(sol))) ** 2))
                    s, c = sol[1::2], sol[2::2]
                    amp = np.hypot(s, c)
                    sigma2 = chi2 / (n - K) if n > K else np.nan
                    i = np.arange(1, K, 2)
                    err = np.sqrt(sigma2 * (s * s * C[i, i] + 2 * s * c * C[i, i + 1] + c * c * C[i + 1, i + 1])) / amp
                    out["theta"][:, iy, ix], out["level"][iy, ix], out["chi2"][iy, ix] = sol, level, chi2
                    out["amplitude"][:, iy, ix], out["phase"][:, iy, ix] = amp, np.arctan2(c, s)
                    out["amplitude_err"][:, iy, ix], out["snr"][:, iy, ix] = err, amp / err
        for key, im in (("amp", out["amplitude"][0]), ("level", out["level"])):
            c, r = centroid_quadratic(im, ap)
            out["centroid_" + key] = np.array([column + c, row + r])
            out["centroid_%s_moments" % key] = np.array([v[0] for v in _moment_centroids(im[None], ap, column, row)])
        out["offset"] = out["centroid_amp"] - out["centroid_level"]
        out["offset_pix"] = float(np.sqrt(np.sum(out["offset"] ** 2)))
        out["status"] = status if status else 3 if np.isnan(out["offset_pix"]) else 0
        return out

    def psf_photometry(self, star_col, star_row, sigma=None, shifts=None, aperture_mask="all", column=0, row=0, use_flux_err=True,
                       prf=None, prf_index=0):
        """Deblended PSF photometry per cadence: the fluxes of up to 8 stars at KNOWN positions and one constant background, by
        weighted linear least squares on every cadence's image (the host mirror of ``DevicePixelCubeBatch.psf_photometry`` and
        its definition, float64 numpy after the float32 load).  The linear form of ``TargetPixelFile.to_lightcurve(method=
        "prf")``: nothing about the PSF is fitted; it is a pixel-integrated Gaussian (``sigma``) or a tabulated PRF (``prf``, below).
        ``star_col`` / ``star_row`` [S]: positions in the coordinates of ``estimate_centroids`` — pixel (iy, ix) covers
        [column + ix - 1/2, column + ix + 1/2] x [row + iy - 1/2, row + iy + 1/2]; a star with a NaN coordinate is left out.
        ``sigma``: a scalar or (sigma_col, sigma_row), pixels.  ``shifts``: None or (shift_col[N], shift_row[N]), added to every
        star's position at that cadence.  With c = star_col[s] + shift_col[n] - column and E(k) = erf((k - 1/2 - c) / (sqrt(2)
        sigma_col)), star s has the column factors (E(ix + 1) - E(ix)) / 2, the row factors likewise, and g[iy, ix] = their
        product.  Per cadence the design is A = [g_0 ... g_{S-1}, 1] over the used pixels: those of ``aperture_mask`` whose flux
        is finite and, with ``use_flux_err``, whose flux_err is finite and > 0; weights w = 1 / flux_err^2, or 1.  G = A^T W A
        is factored by Cholesky without pivoting, in index order; the cadence is singular when a pivot d_k is not finite or d_k
        <= 1e-12 G_kk.  Returns a dict: ``flux`` / ``flux_err`` (S, N) = theta_s and sqrt((G^-1)_ss); ``background`` (N,) =
        theta_S; ``chi2`` (N,) = sum w (y - A theta)^2; ``n_used`` (N,) int32, the used pixels; ``cadence_status`` (N,) int8: 0
        ok, 1 the time or a shift is not finite, 2 n_used < S + 2, 3 singular (a cadence that is not ok is NaN in the four float
        outputs; nothing is raised); ``status``: 0, or 1 when no cadence is ok; ``star_index`` (S,): the stars that took part;
        ``min_pivot_ratio`` (N,): the smallest d_k / G_kk of the factorisation (0 for a pivot that is not finite).
        ``prf``: a ``TabulatedPRF`` in place of ``sigma`` (exactly one of the two, else ``ValueError``), ``prf_index`` its table:
        g[iy, ix] = ``prf.evaluate`` at the star's position (column + ix - star_col[s] - shift_col[n] from the pixel's centre);
        everything else is the same.  A star whose model is zero on every used pixel makes its cadences singular (status 3)."""
        import math
        if (sigma is None) == (prf is None):
            raise ValueError("psf_photometry takes exactly one of sigma and prf")
        if prf is not None:
            if not isinstance(prf, TabulatedPRF):
                raise ValueError("prf must be a TabulatedPRF (got %r)" % (type(prf),))
            prf_index = prf._check_index(prf_index)
        col, rw = np.atleast_1d(np.asarray(star_col, dtype=np.float64)), np.atleast_1d(np.asarray(star_row, dtype=np.float64))
        if col.ndim != 1 or col.shape != rw.shape:
            raise ValueError("star_col and star_row must be 1-D arrays of one length (got %r and %r)" % (col.shape, rw.shape))
        star_index = np.flatnonzero(~(np.isnan(col) | np.isnan(rw)))
        col, rw = col[star_index], rw[star_index]
        S = len(star_index)
        if not 1 <= S <= 8:
            raise ValueError("psf_photometry fits 1 .. 8 stars per cutout (got %d)" % S)
        if not (np.all(np.isfinite(col)) and np.all(np.isfinite(rw))):
            raise ValueError("a star position is infinite")
        if prf is None:
            sig_c, sig_r = _psf_sigma(sigma)
        N, ny, nx = self.shape
        npix, K = ny * nx, S + 1
        if shifts is None:
            dc = dr = np.zeros(1)
        else:
            dc, dr = (np.asarray(a, dtype=np.float64) for a in shifts)
            if dc.shape != (N,) or dr.shape != (N,):
                raise ValueError("shifts must be a pair of arrays of one value per cadence (%d)" % N)
        ap = self._parse_aperture_mask(aperture_mask).reshape(npix)
        erf = np.vectorize(math.erf, otypes=[np.float64])

        def factors(c, sg, n):                                   # c: (S, N or 1) -> (S, N or 1, n)
            E = erf((np.arange(n + 1) - 0.5 - c[..., None]) / (np.sqrt(2.0) * sg))
            return 0.5 * (E[..., 1:] - E[..., :-1])

        with np.errstate(all="ignore"):
            A = np.empty((N, npix, K))
            if prf is None:
                g_col = factors(col[:, None] + dc[None, :] - column, sig_c, nx)
                g_row = factors(rw[:, None] + dr[None, :] - row, sig_r, ny)
                for s in range(S):
                    A[:, :, s] = (g_col[s][:, None, :] * g_row[s][:, :, None]).reshape(-1, npix)
            else:
                g = prf.evaluate((ny, nx), col[:, None] + dc[None, :] - column, rw[:, None] + dr[None, :] - row, prf_index)
                A[:, :, :S] = g.reshape(S, -1, npix).transpose(1, 2, 0)
            A[:, :, S] = 1.0
            y32 = np.asarray(self.flux).reshape(N, npix)
            used = ap[None, :] & np.isfinite(y32)
            if use_flux_err:
                e32 = np.asarray(self.flux_err).reshape(N, npix)
                used &= np.isfinite(e32) & (e32 > 0)
                e = np.where(used, e32, 1).astype(np.float64)
                w = np.where(used, 1.0 / (e * e), 0.0)
            else:
                w = used.astype(np.float64)
            y = np.where(used, y32, 0).astype(np.float64)
            A = np.where(used[:, :, None], A, 0.0)
            WA = A * w[:, :, None]
            G = np.einsum("npi,npj->nij", WA, A)
            rhs = np.einsum("npi,np->ni", WA, y)
            L = np.zeros((N, K, K))
            singular = np.zeros(N, dtype=bool)
            ratio = np.full(N, np.inf)
            for k in range(K):
                d = G[:, k, k].copy()
                for j in range(k):
                    d -= L[:, k, j] * L[:, k, j]
                singular |= ~(np.isfinite(d) & (d > 1e-12 * G[:, k, k]))
                ratio = np.minimum(ratio, np.where(np.isfinite(d) & (G[:, k, k] > 0), d / G[:, k, k], 0.0))
                L[:, k, k] = np.sqrt(d)
                for i in range(k + 1, K):
                    s_ = G[:, k, i].copy()
                    for j in range(k):
                        s_ -= L[:, i, j] * L[:, k, j]
                    L[:, i, k] = s_ / L[:, k, k]
            z, theta, var = np.zeros((N, K)), np.zeros((N, K)), np.zeros((N, K))
            for i in range(K):
                s_ = rhs[:, i].copy()
                for j in range(i):
                    s_ -= L[:, i, j] * z[:, j]
                z[:, i] = s_ / L[:, i, i]
            for i in range(K - 1, -1, -1):
                s_ = z[:, i].copy()
                for j in range(i + 1, K):
                    s_ -= L[:, j, i] * theta[:, j]
                theta[:, i] = s_ / L[:, i, i]
            for k in range(K):                                   # column k of L^-1; (G^-1)_kk = the sum of its squares
                M = np.zeros((N, K))
                M[:, k] = 1.0 / L[:, k, k]
                for i in range(k + 1, K):
                    s_ = np.zeros(N)
                    for j in range(k, i):
                        s_ -= L[:, i, j] * M[:, j]
                    M[:, i] = s_ / L[:, i, i]
                var[:, k] = np.sum(M[:, k:] ** 2, axis=1)
            res = y - np.einsum("npi,ni->np", A, theta)
            chi2 = np.sum(w * res * res, axis=1)
        n_used = used.sum(axis=1).astype(np.int32)
        fin = np.isfinite(self.time) & np.isfinite(dc) & np.isfinite(dr)
        cst = np.where(~fin, 1, np.where(n_used < S + 2, 2, np.where(singular, 3, 0))).astype(np.int8)
        bad = cst != 0
        with np.errstate(all="ignore"):
            err = np.sqrt(var[:, :S]).T
        return {"flux": np.where(bad[None, :], np.nan, theta[:, :S].T), "flux_err": np.where(bad[None, :], np.nan, err),
                "background": np.where(bad, np.nan, theta[:, S]), "chi2": np.where(bad, np.nan, chi2), "n_used": n_used,
                "cadence_status": cst, "status": 0 if np.any(cst == 0) else 1, "star_index": star_index, "min_pivot_ratio": ratio}

    def psf_fit(self, star_col, star_row, sigma=None, shifts0=None, max_iter=10, tol=1e-7, max_step=0.5, max_shift=2.0,
                aperture_mask="all", column=0, row=0, use_flux_err=True, prf=None, prf_index=0):
        """PSF photometry that fits each cadence's pointing shift: per cadence the fluxes of up to 8 stars, one constant
        background and ONE common (column, row) shift u = (dc, dr) of all stars, by variable projection in Kaufman's form (the
        host mirror of ``DevicePixelCubeBatch.psf_fit`` and its definition, float64 numpy after the float32 load).  The
        per-cadence motion shift of ``TargetPixelFile.to_lightcurve(method="prf")``; per-star positions, the PSF width,
        rotation and a background gradient are not fitted.  Stars, ``sigma``, ``aperture_mask``, ``column`` /
        ``row``, the used pixels, the weights w, the star factors g_s at shift u and the design A(u) = [g_0 ... g_{S-1}, 1], K =
        S + 1, are those of ``psf_photometry``; the used pixels do not depend on u.  ``shifts0``: None or (shift_col[N],
        shift_row[N]), the initial shift u0 of every cadence (0 without).  Per cadence, from u = u0, for it = 1 .. ``max_iter``:

        1. G = A^T W A, rhs = A^T W y at u; G = L L^T by the unpivoted Cholesky of ``psf_photometry`` with its pivot cut 1e-12
           G_kk (a failed pivot: status 3); theta = G^-1 rhs.
        2. r = y - A theta; D = [sum_s theta_s dg_s/ddc, sum_s theta_s dg_s/ddr] over the used pixels: the derivative of a
           column factor (E(ix + 1) - E(ix)) / 2 by the centre is -(P(ix + 1) - P(ix)), P(k) = exp(-z_k^2) / (sqrt(2 pi)
           sigma_col), z_k = (k - 1/2 - c) / (sqrt(2) sigma_col); rows likewise.  C = A^T W D (K x 2), E = D^T W D (2 x 2), g =
           D^T W r, S2 = E - (L^-1 C)^T (L^-1 C), factored by the same Cholesky with the pivot cut 1e-12 E_kk (a failed pivot:
           status 3); du = S2^-1 g.
        3. each component of du is clamped to +-``max_step``; u += du; n_iter = it; last_step = max |du| after the clamp.  If
           max |u - u0| > ``max_shift``: status 5, stop.  If ``tol`` > 0 and last_step < ``tol``: converged, stop.

        After ``max_iter`` iterations a cadence that has not converged has status 4 when ``tol`` > 0; ``tol`` = 0 means "take
        exactly ``max_iter`` steps" and is status 0.  A status 0 cadence is evaluated once more at the final u: ``flux``,
        ``flux_err`` = sqrt((G^-1)_ss), ``background`` and ``chi2`` are ``psf_photometry``'s at shifts = u (errors conditional
        on the shift) and ``shift_col_err`` / ``shift_row_err`` = sqrt((S2^-1)_kk) of that evaluation (a failed pivot there:
        status 3).  ``cadence_status`` (N,) int8: 0 ok, 1 the time or u0 is not finite, 2 n_used < S + 4, 3 singular, 4 not
        converged, 5 left ``max_shift``; a cadence that is not ok is NaN in every float output, the shifts included; nothing is
        raised.  Returns the dict of ``psf_photometry`` plus ``shift_col``, ``shift_row``, ``shift_col_err``, ``shift_row_err``
        (N,); ``n_iter`` (N,) int32, the shift updates made, and ``last_step`` (N,), for every cadence (0 / NaN for statuses 1
        and 2); and what the tests' preconditions read: ``steps`` (N, max_iter), the last_step of every iteration, NaN
        afterwards; ``raw_steps`` (N, max_iter, 2), du before the clamp; ``excursion`` (N, max_iter), max |u - u0| after every
        update; ``min_pivot_ratio`` (N,), the smallest d_k / G_kk or d_k / E_kk of every factorisation made (0 for a pivot that
        is not finite).  ``max_iter`` 1 .. 64, ``tol`` finite and >= 0, ``max_step`` and ``max_shift`` > 0 (``ValueError``).
        ``prf``: a ``TabulatedPRF`` in place of ``sigma`` (exactly one of the two, else ``ValueError``; ``prf_index`` its table,
        ``ValueError`` without ``prf``).  Steps 1 to 3 hold word for word with the design columns A_s = P_s, ``prf.evaluate`` at
        (col_s + dc - column, row_s + dr - row), and D = [sum_s theta_s dP_s/dc, sum_s theta_s dP_s/dr], s in index order,
        from ``prf.evaluate_with_gradient``: a shift and a centre enter as one sum, so the derivative by the shift is the
        derivative by the centre.  Everything else is the same; a cadence whose stars all have a zero model or a zero
        derivative on the used pixels fails a pivot cut (status 3)."""
        import math
        if (sigma is None) == (prf is None):
            raise ValueError("psf_fit takes exactly one of sigma and prf")
        if prf is None:
            if prf_index is not None and not (np.ndim(prf_index) == 0 and prf_index == 0):
                raise ValueError("prf_index needs prf")
        else:
            if not isinstance(prf, TabulatedPRF):
                raise ValueError("prf must be a TabulatedPRF (got %r)" % (type(prf),))
            prf_index = prf._check_index(prf_index)
        col, rw = np.atleast_1d(np.asarray(star_col, dtype=np.float64)), np.atleast_1d(np.asarray(star_row, dtype=np.float64))
        if col.ndim != 1 or col.shape != rw.shape:
            raise ValueError("star_col and star_row must be 1-D arrays of one length (got %r and %r)" % (col.shape, rw.shape))
        star_index = np.flatnonzero(~(np.isnan(col) | np.isnan(rw)))
        col, rw = col[star_index], rw[star_index]
        S = len(star_index)
        if not 1 <= S <= 8:
            raise ValueError("psf_fit fits 1 .. 8 stars per cutout (got %d)" % S)
        if not (np.all(np.isfinite(col)) and np.all(np.isfinite(rw))):
            raise ValueError("a star position is infinite")
        if prf is None:
            sig_c, sig_r = _psf_sigma(sigma)
        max_iter, tol, max_step, max_shift = _psf_fit_parameters(max_iter, tol, max_step, max_shift)
        N, ny, nx = self.shape
        npix, K = ny * nx, S + 1
        if shifts0 is None:
            u0 = np.zeros((N, 2))
        else:
            u0 = np.stack([np.asarray(a, dtype=np.float64) for a in shifts0], axis=-1)
            if len(shifts0) != 2 or u0.shape != (N, 2):
                raise ValueError("shifts0 must be a pair of arrays of one value per cadence (%d)" % N)
        ap = self._parse_aperture_mask(aperture_mask).reshape(npix)
        erf = np.vectorize(math.erf, otypes=[np.float64])
        y32 = np.asarray(self.flux).reshape(N, npix)
        used = ap[None, :] & np.isfinite(y32)
        with np.errstate(all="ignore"):
            if use_flux_err:
                e32 = np.asarray(self.flux_err).reshape(N, npix)
                used &= np.isfinite(e32) & (e32 > 0)
                e = np.where(used, e32, 1).astype(np.float64)
                w_all = np.where(used, 1.0 / (e * e), 0.0)
            else:
                w_all = used.astype(np.float64)
        y_all = np.where(used, y32, 0).astype(np.float64)
        n_used = used.sum(axis=1).astype(np.int32)

        def tables(c, sg, n):                                    # c: (S, M) -> factors and their derivatives by c, (S, M, n)
            z = (np.arange(n + 1) - 0.5 - c[..., None]) / (np.sqrt(2.0) * sg)
            E, P = erf(z), np.exp(-z * z) / (np.sqrt(2.0 * np.pi) * sg)
            return 0.5 * (E[..., 1:] - E[..., :-1]), -(P[..., 1:] - P[..., :-1])

        cholesky, forward, backward = _psf_cholesky, _psf_forward, _psf_backward

        def gaussian_model(u, A, Ac, Ar):
            """The star columns of A (M, npix, K) and their derivatives by (dc, dr), (M, npix, S) each, at the shifts u."""
            M = len(u)
            g_col, d_col = tables(col[:, None] + u[None, :, 0] - column, sig_c, nx)
            g_row, d_row = tables(rw[:, None] + u[None, :, 1] - row, sig_r, ny)
            for s in range(S):
                A[:, :, s] = (g_col[s][:, None, :] * g_row[s][:, :, None]).reshape(M, npix)
                Ac[:, :, s] = (d_col[s][:, None, :] * g_row[s][:, :, None]).reshape(M, npix)
                Ar[:, :, s] = (g_col[s][:, None, :] * d_row[s][:, :, None]).reshape(M, npix)

        def tabulated_model(u, A, Ac, Ar):
            M = len(u)
            P, Pc, Pr = prf.evaluate_with_gradient((ny, nx), col[:, None] + u[None, :, 0] - column,
                                                   rw[:, None] + u[None, :, 1] - row, prf_index)
            for dst, src in ((A, P), (Ac, Pc), (Ar, Pr)):
                dst[:, :, :S] = src.reshape(S, M, npix).transpose(1, 2, 0)

        model = gaussian_model if prf is None else tabulated_model

        def evaluate(idx, u):
            """The cadences idx at the shifts u (M, 2) -> theta (M, K), L, L2, g (M, 2), chi2, singular, pivot ratio."""
            M = len(idx)
            w, y, keep = w_all[idx], y_all[idx], used[idx]
            A, Ac, Ar = np.empty((M, npix, K)), np.empty((M, npix, S)), np.empty((M, npix, S))
            model(u, A, Ac, Ar)
            A[:, :, S] = 1.0
            A = np.where(keep[:, :, None], A, 0.0)
            WA = A * w[:, :, None]
            G = np.einsum("npi,npj->nij", WA, A)
            rhs = np.einsum("npi,np->ni", WA, y)
            L, singular, ratio = cholesky(G, np.einsum("nii->ni", G))
            theta = backward(L, forward(L, rhs[:, :, None]))[:, :, 0]
            res = y - np.einsum("npi,ni->np", A, theta)
            D = np.stack([np.einsum("nps,ns->np", Ac, theta[:, :S]), np.einsum("nps,ns->np", Ar, theta[:, :S])], axis=2)
            D = np.where(keep[:, :, None], D, 0.0)
            WD = D * w[:, :, None]
            Y = forward(L, np.einsum("npi,npj->nij", A, WD))
            E = np.einsum("npi,npj->nij", WD, D)
            L2, singular2, ratio2 = cholesky(E - np.einsum("nki,nkj->nij", Y, Y), np.einsum("nii->ni", E))
            return dict(theta=theta, L=L, L2=L2, g=np.einsum("npi,np->ni", WD, res), chi2=np.sum(w * res * res, axis=1),
                        singular=singular | singular2, ratio=np.minimum(ratio, ratio2))

        fin = np.isfinite(self.time) & np.all(np.isfinite(u0), axis=1)
        cst = np.where(~fin, 1, np.where(n_used < S + 4, 2, 0)).astype(np.int8)
        u = u0.copy()
        n_iter, last_step = np.zeros(N, dtype=np.int32), np.full(N, np.nan)
        steps, raw_steps, excursion = np.full((N, max_iter), np.nan), np.full((N, max_iter, 2), np.nan), np.full((N, max_iter), np.nan)
        ratio = np.full(N, np.inf)
        running = cst == 0
        final = np.zeros(N, dtype=bool)                          # stopped and ok: the evaluation at the final u is to come
        with np.errstate(all="ignore"):
            for it in range(1, max_iter + 1):
                idx = np.flatnonzero(running)
                if not len(idx):
                    break
                ev = evaluate(idx, u[idx])
                ratio[idx] = np.minimum(ratio[idx], ev["ratio"])
                du = backward(ev["L2"], forward(ev["L2"], ev["g"][:, :, None]))[:, :, 0]
                go = ~ev["singular"]
                cst[idx[~go]] = 3
                running[idx[~go]] = False
                idx, du = idx[go], du[go]
                raw_steps[idx, it - 1] = du
                du = np.where(du > max_step, max_step, np.where(du < -max_step, -max_step, du))
                u[idx] += du
                n_iter[idx] = it
                a0, a1 = np.abs(du[:, 0]), np.abs(du[:, 1])
                last_step[idx] = steps[idx, it - 1] = np.where(a0 > a1, a0, a1)
                a0, a1 = np.abs(u[idx, 0] - u0[idx, 0]), np.abs(u[idx, 1] - u0[idx, 1])
                exc = excursion[idx, it - 1] = np.where(a0 > a1, a0, a1)
                left = exc > max_shift
                conv = ~left & (tol > 0) & (last_step[idx] < tol)
                cst[idx[left]] = 5
                running[idx[left | conv]] = False
                final[idx[conv]] = True
            if tol > 0:
                cst[running] = 4
            else:
                final |= running
            flux, err = np.full((S, N), np.nan), np.full((S, N), np.nan)
            out = {k: np.full(N, np.nan) for k in ("background", "chi2", "shift_col", "shift_row", "shift_col_err", "shift_row_err")}
            idx = np.flatnonzero(final)
            if len(idx):
                ev = evaluate(idx, u[idx])
                ratio[idx] = np.minimum(ratio[idx], ev["ratio"])
                cst[idx[ev["singular"]]] = 3
                eye = np.broadcast_to(np.eye(K)[None], (len(idx), K, K))
                var = np.sum(forward(ev["L"], eye.copy()) ** 2, axis=1)          # (G^-1)_kk = the squares of column k of L^-1
                var2 = np.sum(forward(ev["L2"], np.broadcast_to(np.eye(2)[None], (len(idx), 2, 2)).copy()) ** 2, axis=1)
                ok = ~ev["singular"]
                at = idx[ok]
                flux[:, at], err[:, at] = ev["theta"][ok, :S].T, np.sqrt(var[ok, :S]).T
                out["background"][at], out["chi2"][at] = ev["theta"][ok, S], ev["chi2"][ok]
                out["shift_col"][at], out["shift_row"][at] = u[at, 0], u[at, 1]
                out["shift_col_err"][at], out["shift_row_err"][at] = np.sqrt(var2[ok, 0]), np.sqrt(var2[ok, 1])
        out.update(flux=flux, flux_err=err, n_used=n_used, cadence_status=cst, status=0 if np.any(cst == 0) else 1,
                   star_index=star_index, min_pivot_ratio=ratio, n_iter=n_iter, last_step=last_step, steps=steps,
                   raw_steps=raw_steps, excursion=excursion)
        return out

    def psf_width(self, star_col, star_row, sigma0, shifts=None, cadence_mask=None, max_iter=20, tol=1e-6, max_step=0.25,
                  min_sigma=0.2, max_sigma=5.0, aperture_mask="all", column=0, row=0, use_flux_err=True):
        """The PSF width of the cutout, fitted: ONE pair v = (sigma_col, sigma_row) shared by every cadence, by variable
        projection in Kaufman's form with the linear unknowns (the fluxes of up to 8 stars and a background PER CADENCE)
        projected out (the host mirror of ``DevicePixelCubeBatch.psf_width`` and its definition, float64 numpy after the float32
        load).  The PSF scale of ``TargetPixelFile.to_lightcurve(method="prf")``; the third step of the chain ``psf_fit(sigma
        guess)`` -> ``psf_width(shifts=)`` -> ``psf_fit(sigma)`` / ``psf_photometry(sigma, shifts)``.  Stars, ``aperture_mask``,
        ``column`` / ``row``, the PSF, the used pixels, the weights w, the design A = [g_0 ... g_{S-1}, 1], K = S + 1, the
        Cholesky and its pivot cut 1e-12 G_kk are those of ``psf_photometry``.  ``shifts``: None or (shift_col[N], shift_row[N]),
        added to every star's position as in ``psf_photometry``.  ``cadence_mask``: None or bool (N,), the cadences the width
        is fitted on.  ``sigma0``: a scalar or (sigma_col, sigma_row), the start.

        A cadence is ELIGIBLE when ``cadence_mask`` selects it, its time and its shift are finite and n_used >= S + 2; that
        does not depend on v.  One EVALUATION at v, per eligible cadence: G = A^T W A, rhs = A^T W y, G = L L^T, theta = G^-1
        rhs, r = y - A theta; D = [sum_s theta_s dg_s/dsigma_col, sum_s theta_s dg_s/dsigma_row] over the used pixels, where the
        derivative of a column factor (erf(z_{k+1}) - erf(z_k)) / 2, z_k = (k - 1/2 - c) / (sqrt(2) sigma_col), by sigma_col is
        -(Q(k + 1) - Q(k)), Q(k) = (k - 1/2 - c) exp(-z_k^2) / (sqrt(2 pi) sigma_col^2), rows likewise; C = A^T W D, E = D^T W
        D, g_n = D^T W r, S2_n = E - (L^-1 C)^T (L^-1 C), chi2_n = sum w r^2.  A cadence whose G fails a pivot is singular at
        this evaluation and contributes nothing.  The cutout's sums g = sum g_n, H = sum S2_n, chi2, n_cadences and n_pixels =
        sum n_used run over the contributing cadences in an order fixed by N alone.

        From v = ``sigma0``, for it = 1 .. ``max_iter``: (1) evaluate at v; (2) n_cadences == 0: status 1, stop; (3) H = L2
        L2^T by the 2 x 2 unpivoted Cholesky, singular when H_00 is not finite and > 0 or d_11 is not finite and > 1e-12 H_11:
        status 3, stop; (4) dv = H^-1 g, each component clamped to +-``max_step``; (5) v += dv, n_iter = it, last_step = max
        |dv|; (6) a component of v not in [``min_sigma``, ``max_sigma``]: status 5, stop; (7) ``tol`` > 0 and last_step <
        ``tol``: converged.  After ``max_iter`` steps without convergence the status is 4, but ``tol`` = 0 means "exactly
        ``max_iter`` steps" and is status 0.  A status 0 cutout is evaluated once more at its final v (no cadence there: status
        1; H singular: status 3), which gives ``sigma`` (2,) = v, ``sigma_err`` (2,) = sqrt((H^-1)_kk) (not scaled by chi2,
        conditional on the shifts), ``sigma_cov`` = (H^-1)_01, ``chi2``.  A failed cutout is NaN in those four; nothing is
        raised.  Always returned: ``status``; ``n_cadences`` and ``n_pixels`` (int64) of the last evaluation made; ``n_iter``
        and ``last_step`` (NaN before the first update); ``trace`` (max_iter + 1, 2): row k is the v of evaluation k + 1, NaN
        beyond the evaluations made — the final evaluation is made at row n_iter, so a status 0 cutout has n_iter + 1 rows
        and a v that left the bounds (status 5) is not in it; ``cadence_status`` (N,) int8 from the last evaluation made, in
        this order of precedence: 6 not selected by ``cadence_mask``, 1 the time or a shift is not finite, 2 n_used < S + 2, 3
        singular, 0 contributed; ``n_used`` (N,) int32; ``star_index``; and what the tests' preconditions read: ``steps``
        (max_iter,), ``raw_steps`` (max_iter, 2) before the clamp, ``visited`` (max_iter, 2), v after every update, and
        ``min_pivot_ratio``, the smallest d_k / G_kk (eligible cadences) or d_k / H_kk of every factorisation made.
        ``ValueError``: ``max_iter`` outside 1 .. 64, ``tol`` not finite or < 0, ``max_step`` not > 0, not 0 < ``min_sigma`` <=
        ``sigma0`` <= ``max_sigma`` or a bound not finite."""
        col, rw = np.atleast_1d(np.asarray(star_col, dtype=np.float64)), np.atleast_1d(np.asarray(star_row, dtype=np.float64))
        if col.ndim != 1 or col.shape != rw.shape:
            raise ValueError("star_col and star_row must be 1-D arrays of one length (got %r and %r)" % (col.shape, rw.shape))
        star_index = np.flatnonzero(~(np.isnan(col) | np.isnan(rw)))
        col, rw = col[star_index], rw[star_index]
        S = len(star_index)
        if not 1 <= S <= 8:
            raise ValueError("psf_width fits 1 .. 8 stars per cutout (got %d)" % S)
        if not (np.all(np.isfinite(col)) and np.all(np.isfinite(rw))):
            raise ValueError("a star position is infinite")
        v = np.array(_psf_sigma(sigma0))
        max_iter, tol, max_step, min_sigma, max_sigma = _psf_width_parameters(max_iter, tol, max_step, min_sigma, max_sigma, v)
        N, ny, nx = self.shape
        npix, K = ny * nx, S + 1
        if shifts is None:
            dc = dr = np.zeros(N)
        else:
            if len(shifts) != 2:
                raise ValueError("shifts must be a pair (shift_col, shift_row)")
            dc, dr = (np.asarray(a, dtype=np.float64) for a in shifts)
            if dc.shape != (N,) or dr.shape != (N,):
                raise ValueError("shifts must be a pair of arrays of one value per cadence (%d)" % N)
        if cadence_mask is None:
            selected = np.ones(N, dtype=bool)
        else:
            selected = np.asarray(cadence_mask)
            if selected.dtype != bool or selected.shape != (N,):
                raise ValueError("cadence_mask must be a bool array of one value per cadence (%d)" % N)
        ap = self._parse_aperture_mask(aperture_mask).reshape(npix)
        y32 = np.asarray(self.flux).reshape(N, npix)
        used = ap[None, :] & np.isfinite(y32)
        with np.errstate(all="ignore"):
            if use_flux_err:
                e32 = np.asarray(self.flux_err).reshape(N, npix)
                used &= np.isfinite(e32) & (e32 > 0)
                e = np.where(used, e32, 1).astype(np.float64)
                w_all = np.where(used, 1.0 / (e * e), 0.0)
            else:
                w_all = used.astype(np.float64)
        y_all = np.where(used, y32, 0).astype(np.float64)
        n_used = used.sum(axis=1).astype(np.int32)
        base = np.where(~selected, 6, np.where(~(np.isfinite(self.time) & np.isfinite(dc) & np.isfinite(dr)), 1,
                                               np.where(n_used < S + 2, 2, 0))).astype(np.int8)
        idx = np.flatnonzero(base == 0)                         # the eligible cadences
        w, y, keep = w_all[idx], y_all[idx], used[idx]
        M = len(idx)

        def evaluate(v):
            """-> g (2,), H (2, 2), chi2, n_cadences, n_pixels, cadence_status (N,), the smallest pivot ratio of G."""
            g_col, d_col = _psf_width_tables(col[:, None] + dc[None, idx] - column, v[0], nx)
            g_row, d_row = _psf_width_tables(rw[:, None] + dr[None, idx] - row, v[1], ny)
            A, Ac, Ar = np.empty((M, npix, K)), np.empty((M, npix, S)), np.empty((M, npix, S))
            for s in range(S):
                A[:, :, s] = (g_col[s][:, None, :] * g_row[s][:, :, None]).reshape(M, npix)
                Ac[:, :, s] = (d_col[s][:, None, :] * g_row[s][:, :, None]).reshape(M, npix)
                Ar[:, :, s] = (g_col[s][:, None, :] * d_row[s][:, :, None]).reshape(M, npix)
            A[:, :, S] = 1.0
            A = np.where(keep[:, :, None], A, 0.0)
            WA = A * w[:, :, None]
            G = np.einsum("npi,npj->nij", WA, A)
            L, singular, ratio = _psf_cholesky(G, np.einsum("nii->ni", G))
            theta = _psf_backward(L, _psf_forward(L, np.einsum("npi,np->ni", WA, y)[:, :, None]))[:, :, 0]
            res = y - np.einsum("npi,ni->np", A, theta)
            D = np.stack([np.einsum("nps,ns->np", Ac, theta[:, :S]), np.einsum("nps,ns->np", Ar, theta[:, :S])], axis=2)
            D = np.where(keep[:, :, None], D, 0.0)
            WD = D * w[:, :, None]
            Y = _psf_forward(L, np.einsum("npi,npj->nij", A, WD))
            S2 = np.einsum("npi,npj->nij", WD, D) - np.einsum("nki,nkj->nij", Y, Y)
            ok = ~singular
            cst = base.copy()
            cst[idx[singular]] = 3
            return dict(g=np.where(ok[:, None], np.einsum("npi,np->ni", WD, res), 0.0).sum(axis=0),
                        H=np.where(ok[:, None, None], S2, 0.0).sum(axis=0), chi2=np.where(ok, np.sum(w * res * res, axis=1), 0.0).sum(),
                        n_cadences=int(ok.sum()), n_pixels=int(n_used[idx][ok].sum()), cadence_status=cst,
                        ratio=ratio.min() if M else np.inf)

        def factor(H):                                           # the 2 x 2 Cholesky -> l00, l10, l11, singular, pivot ratio
            singular = not (np.isfinite(H[0, 0]) and H[0, 0] > 0)
            l00 = np.sqrt(H[0, 0])
            l10 = H[0, 1] / l00
            d11 = H[1, 1] - l10 * l10
            singular = singular or not (np.isfinite(d11) and d11 > 1e-12 * H[1, 1])
            return l00, l10, np.sqrt(d11), singular, d11 / H[1, 1] if np.isfinite(d11) and H[1, 1] > 0 else 0.0

        n_iter, last_step, status = 0, np.nan, 4
        trace = np.full((max_iter + 1, 2), np.nan)
        steps, raw_steps, visited = np.full(max_iter, np.nan), np.full((max_iter, 2), np.nan), np.full((max_iter, 2), np.nan)
        ratio = np.inf
        out = dict(sigma=np.full(2, np.nan), sigma_err=np.full(2, np.nan), sigma_cov=np.nan, chi2=np.nan)
        with np.errstate(all="ignore"):
            for it in range(1, max_iter + 1):
                ev = evaluate(v)
                trace[it - 1] = v
                ratio = min(ratio, ev["ratio"])
                if ev["n_cadences"] == 0:
                    status = 1
                    break
                l00, l10, l11, singular, r2 = factor(ev["H"])
                ratio = min(ratio, r2)
                if singular:
                    status = 3
                    break
                z0 = ev["g"][0] / l00
                z1 = (ev["g"][1] - l10 * z0) / l11
                dv1 = z1 / l11
                dv = np.array([(z0 - l10 * dv1) / l00, dv1])
                raw_steps[it - 1] = dv
                dv = np.where(dv > max_step, max_step, np.where(dv < -max_step, -max_step, dv))
                v = v + dv
                n_iter, visited[it - 1] = it, v
                last_step = steps[it - 1] = abs(dv[0]) if abs(dv[0]) > abs(dv[1]) else abs(dv[1])
                if not (np.all(v >= min_sigma) and np.all(v <= max_sigma)):
                    status = 5
                    break
                if tol > 0 and last_step < tol:
                    status = 0
                    break
            if status == 4 and tol == 0:
                status = 0
            if status == 0:
                ev = evaluate(v)
                trace[n_iter] = v
                ratio = min(ratio, ev["ratio"])
                if ev["n_cadences"] == 0:
                    status = 1
                else:
                    l00, l10, l11, singular, r2 = factor(ev["H"])
                    ratio = min(ratio, r2)
                    if singular:
                        status = 3
                    else:
                        m00, m11 = 1.0 / l00, 1.0 / l11
                        m10 = -l10 * m00 * m11
                        out = dict(sigma=v.copy(), sigma_err=np.array([np.sqrt(m00 * m00 + m10 * m10), m11]), sigma_cov=m10 * m11,
                                   chi2=float(ev["chi2"]))
        out.update(status=status, n_cadences=ev["n_cadences"], n_pixels=ev["n_pixels"], n_iter=n_iter, last_step=float(last_step),
                   trace=trace, cadence_status=ev["cadence_status"], n_used=n_used, star_index=star_index, steps=steps,
                   raw_steps=raw_steps, visited=visited, min_pivot_ratio=float(ratio))
        return out

    def psf_positions(self, star_col, star_row, sigma, shifts=None, cadence_mask=None, fit_star=None, max_iter=20, tol=1e-6,
                      max_step=0.25, max_offset=1.0, aperture_mask="all", column=0, row=0, use_flux_err=True):
        """The positions of the cutout's stars, fitted: ONE (column, row) per fitted star, shared by every cadence, by variable
        projection in Kaufman's form with the linear unknowns (the fluxes of up to 8 stars and a background PER CADENCE)
        projected out (the host mirror of ``DevicePixelCubeBatch.psf_positions`` and its definition, float64 numpy after the
        float32 load).  The last unknown of ``TargetPixelFile.to_lightcurve(method="prf")`` that the PSF calls took as given; the
        chain is ``psf_fit(guess)`` -> ``psf_positions(shifts=)`` -> ``psf_width(shifts=)`` -> ``psf_fit`` / ``psf_photometry``.
        Stars (NaN = an empty slot), ``aperture_mask``, ``column`` / ``row``, ``sigma`` (given, not fitted), the PSF, the used
        pixels, the weights w, the design A = [g_0 ... g_{S-1}, 1], K = S + 1, the Cholesky and its pivot cut 1e-12 G_kk are
        those of ``psf_photometry``; ``shifts`` and ``cadence_mask`` those of ``psf_width``.  ``fit_star``: None (every star
        present is fitted) or a bool array over the slots; a star that is not fitted stays at its given position (a faint
        neighbour left at its catalogue value); no fitted star is a ``ValueError``.

        THE FIT IS CONDITIONAL ON THE SHIFTS (and on the width): a translation common to all stars is the same model as a
        constant added to every shift, the call never frees both, and ``fit_star`` can pin an anchor star.

        The unknowns v are (column, row) of the fitted stars in slot order, v[2j] the column and v[2j + 1] the row of the j-th
        fitted star, P = 2 x their number <= 16; v starts at the given positions.  A cadence is ELIGIBLE when ``cadence_mask``
        selects it, its time and its shift are finite and n_used >= S + 2; that does not depend on v.  One EVALUATION at v, per
        eligible cadence: G = A^T W A, rhs = A^T W y, G = L L^T, theta = G^-1 rhs, r = y - A theta; D has one column per
        unknown, for star s theta_s (dg_s^col/dc) g_s^row and theta_s g_s^col (dg_s^row/dc) over the used pixels, where the
        derivative of a factor (erf(z_{k+1}) - erf(z_k)) / 2, z_k = (k - 1/2 - c) / (sqrt(2) sigma), by its centre c is -(P(k +
        1) - P(k)), P(k) = exp(-z_k^2) / (sqrt(2 pi) sigma) (``psf_fit``'s derivative by the shift); C = A^T W D (K x P), E =
        D^T W D, g_n = D^T W r, S2_n = E - (L^-1 C)^T (L^-1 C), chi2_n = sum w r^2.  The columns of every star are formed; the
        Schur complement over the fitted subset is exactly the submatrix of S2_n.  A cadence whose G fails a pivot is singular
        at this evaluation and contributes nothing.  The cutout's sums g = sum g_n, H = sum S2_n, chi2, n_cadences and
        n_pixels = sum n_used run over the contributing cadences in an order fixed by N alone.

        For it = 1 .. ``max_iter``: (1) evaluate at v; (2) n_cadences == 0: status 1, stop; (3) H (the fitted rows and
        columns) = L2 L2^T by the P x P unpivoted Cholesky, singular when a pivot d_k is not finite and > 1e-12 H_kk: status 3,
        stop; (4) dv = H^-1 g, each component clamped to +-``max_step``; (5) v += dv, n_iter = it, last_step = max |dv|; (6) a
        component of v farther than ``max_offset`` from its start: status 5, stop; (7) ``tol`` > 0 and last_step < ``tol``:
        converged.  After ``max_iter`` steps without convergence the status is 4, but ``tol`` = 0 means "exactly ``max_iter``
        steps" and is status 0.  A status 0 cutout is evaluated once more at its final v (no cadence there: status 1; H
        singular: status 3) for the outputs, all in the caller's slot layout (S_max slots): ``star_col`` / ``star_row`` (S_max,):
        the fitted values, the given value bit for bit for a star that is not fitted, NaN in an empty slot; ``star_col_err`` /
        ``star_row_err`` = sqrt((H^-1)_kk), not scaled by chi2 and conditional on shifts and width, NaN where the star is not
        fitted; ``position_cov`` (2 S_max, 2 S_max) = H^-1 at index 2 slot + axis, NaN rows and columns where the star is not
        fitted; ``chi2``.  A failed cutout is NaN in the fitted stars' positions, their errors, ``position_cov`` and ``chi2``;
        nothing is raised.  Always returned: ``status``; ``n_cadences`` and ``n_pixels`` (int64) of the last evaluation made;
        ``n_iter`` and ``last_step`` (NaN before the first update); ``trace`` (max_iter + 1, 2 S_max): row k holds the
        positions of evaluation k + 1 at index 2 slot + axis (a star that is not fitted at its given value, NaN in an empty
        slot), NaN beyond the evaluations made — the final evaluation is made at row n_iter, so a status 0 cutout has n_iter +
        1 rows and a v that left ``max_offset`` (status 5) is not in it; ``cadence_status`` (N,) int8 from the last evaluation
        made, in this order of precedence: 6 not selected by ``cadence_mask``, 1 the time or a shift is not finite, 2 n_used <
        S + 2, 3 singular, 0 contributed; ``n_used`` (N,) int32; ``star_index`` and ``fitted_index`` (the slots of the stars
        and of the fitted stars); and what the tests' preconditions read: ``steps`` (max_iter,), ``raw_steps`` (max_iter, P)
        before the clamp, ``visited`` (max_iter, P), v after every update, ``start`` (P,), ``min_pivot_ratio``, the smallest
        d_k / G_kk (eligible cadences) or d_k / H_kk of every factorisation made, and ``first_gradient`` (2 S,) and
        ``first_hessian`` (2 S, 2 S), g and H of the first evaluation over ALL the stars' columns (index 2 star + axis).
        ``ValueError``: the argument errors of ``psf_width``, ``max_offset`` not > 0, a ``fit_star`` of another shape or
        dtype, or no fitted star."""
        col_in, rw_in = np.atleast_1d(np.asarray(star_col, dtype=np.float64)), np.atleast_1d(np.asarray(star_row, dtype=np.float64))
        if col_in.ndim != 1 or col_in.shape != rw_in.shape:
            raise ValueError("star_col and star_row must be 1-D arrays of one length (got %r and %r)" % (col_in.shape, rw_in.shape))
        S_max = len(col_in)
        star_index = np.flatnonzero(~(np.isnan(col_in) | np.isnan(rw_in)))
        col, rw = col_in[star_index], rw_in[star_index]
        S = len(star_index)
        if not 1 <= S <= 8:
            raise ValueError("psf_positions fits 1 .. 8 stars per cutout (got %d)" % S)
        if not (np.all(np.isfinite(col)) and np.all(np.isfinite(rw))):
            raise ValueError("a star position is infinite")
        if fit_star is None:
            fit = np.ones(S_max, dtype=bool)
        else:
            fit = np.asarray(fit_star)
            if fit.dtype != bool or fit.shape != (S_max,):
                raise ValueError("fit_star must be a bool array of one value per slot (%d)" % S_max)
        fitted = np.flatnonzero(fit[star_index])                # among the stars present
        if len(fitted) == 0:
            raise ValueError("no star of the cutout is fitted")
        fitted_index = star_index[fitted]
        sg = _psf_sigma(sigma)
        max_iter, tol, max_step, max_offset = _psf_positions_parameters(max_iter, tol, max_step, max_offset)
        N, ny, nx = self.shape
        npix, K, P = ny * nx, S + 1, 2 * len(fitted)
        sel = np.stack([2 * fitted, 2 * fitted + 1], axis=1).reshape(-1)       # the fitted columns among the 2 S
        if shifts is None:
            dc = dr = np.zeros(N)
        else:
            if len(shifts) != 2:
                raise ValueError("shifts must be a pair (shift_col, shift_row)")
            dc, dr = (np.asarray(a, dtype=np.float64) for a in shifts)
            if dc.shape != (N,) or dr.shape != (N,):
                raise ValueError("shifts must be a pair of arrays of one value per cadence (%d)" % N)
        if cadence_mask is None:
            selected = np.ones(N, dtype=bool)
        else:
            selected = np.asarray(cadence_mask)
            if selected.dtype != bool or selected.shape != (N,):
                raise ValueError("cadence_mask must be a bool array of one value per cadence (%d)" % N)
        ap = self._parse_aperture_mask(aperture_mask).reshape(npix)
        y32 = np.asarray(self.flux).reshape(N, npix)
        used = ap[None, :] & np.isfinite(y32)
        with np.errstate(all="ignore"):
            if use_flux_err:
                e32 = np.asarray(self.flux_err).reshape(N, npix)
                used &= np.isfinite(e32) & (e32 > 0)
                e = np.where(used, e32, 1).astype(np.float64)
                w_all = np.where(used, 1.0 / (e * e), 0.0)
            else:
                w_all = used.astype(np.float64)
        y_all = np.where(used, y32, 0).astype(np.float64)
        n_used = used.sum(axis=1).astype(np.int32)
        base = np.where(~selected, 6, np.where(~(np.isfinite(self.time) & np.isfinite(dc) & np.isfinite(dr)), 1,
                                               np.where(n_used < S + 2, 2, 0))).astype(np.int8)
        idx = np.flatnonzero(base == 0)                         # the eligible cadences
        w, y, keep = w_all[idx], y_all[idx], used[idx]
        M = len(idx)

        def evaluate(pos):
            """pos (2 S,): every star's (column, row) -> g (2 S,), H (2 S, 2 S), chi2, the counts, cadence_status, pivot ratio."""
            g_col, d_col = _psf_centre_tables(pos[0::2, None] + dc[None, idx] - column, sg[0], nx)
            g_row, d_row = _psf_centre_tables(pos[1::2, None] + dr[None, idx] - row, sg[1], ny)
            A, Dp = np.empty((M, npix, K)), np.empty((M, npix, 2 * S))
            for s in range(S):
                A[:, :, s] = (g_col[s][:, None, :] * g_row[s][:, :, None]).reshape(M, npix)
                Dp[:, :, 2 * s] = (d_col[s][:, None, :] * g_row[s][:, :, None]).reshape(M, npix)
                Dp[:, :, 2 * s + 1] = (g_col[s][:, None, :] * d_row[s][:, :, None]).reshape(M, npix)
            A[:, :, S] = 1.0
            A = np.where(keep[:, :, None], A, 0.0)
            WA = A * w[:, :, None]
            G = np.einsum("npi,npj->nij", WA, A)
            L, singular, ratio = _psf_cholesky(G, np.einsum("nii->ni", G))
            theta = _psf_backward(L, _psf_forward(L, np.einsum("npi,np->ni", WA, y)[:, :, None]))[:, :, 0]
            res = y - np.einsum("npi,ni->np", A, theta)
            D = np.where(keep[:, :, None], Dp * np.repeat(theta[:, :S], 2, axis=1)[:, None, :], 0.0)
            WD = D * w[:, :, None]
            Y = _psf_forward(L, np.einsum("npi,npj->nij", A, WD))
            S2 = np.einsum("npi,npj->nij", WD, D) - np.einsum("nki,nkj->nij", Y, Y)
            ok = ~singular
            cst = base.copy()
            cst[idx[singular]] = 3
            return dict(g=np.where(ok[:, None], np.einsum("npi,np->ni", WD, res), 0.0).sum(axis=0),
                        H=np.where(ok[:, None, None], S2, 0.0).sum(axis=0), chi2=np.where(ok, np.sum(w * res * res, axis=1), 0.0).sum(),
                        n_cadences=int(ok.sum()), n_pixels=int(n_used[idx][ok].sum()), cadence_status=cst,
                        ratio=ratio.min() if M else np.inf)

        def factor(H):                                           # the fitted rows and columns -> L2, singular, pivot ratio
            Hf = H[np.ix_(sel, sel)]
            L2, singular, r2 = _psf_cholesky(Hf[None], np.diag(Hf)[None])
            return L2, bool(singular[0]), float(r2[0])

        def slots(pos):                                          # (2 S,) -> (2 S_max,) at index 2 slot + axis, NaN in empty slots
            out = np.full(2 * S_max, np.nan)
            out[2 * star_index], out[2 * star_index + 1] = pos[0::2], pos[1::2]
            return out

        pos = np.stack([col, rw], axis=1).reshape(-1)            # every star's position; the fitted ones move
        start = pos[sel].copy()
        n_iter, last_step, status = 0, np.nan, 4
        trace = np.full((max_iter + 1, 2 * S_max), np.nan)
        steps, raw_steps, visited = np.full(max_iter, np.nan), np.full((max_iter, P), np.nan), np.full((max_iter, P), np.nan)
        ratio, first = np.inf, None
        out = dict(star_col=np.where(fit, np.nan, col_in), star_row=np.where(fit, np.nan, rw_in), star_col_err=np.full(S_max, np.nan),
                   star_row_err=np.full(S_max, np.nan), position_cov=np.full((2 * S_max, 2 * S_max), np.nan), chi2=np.nan)
        with np.errstate(all="ignore"):
            for it in range(1, max_iter + 1):
                ev = evaluate(pos)
                if first is None:
                    first = ev
                trace[it - 1] = slots(pos)
                ratio = min(ratio, ev["ratio"])
                if ev["n_cadences"] == 0:
                    status = 1
                    break
                L2, singular, r2 = factor(ev["H"])
                ratio = min(ratio, r2)
                if singular:
                    status = 3
                    break
                dv = _psf_backward(L2, _psf_forward(L2, ev["g"][sel][None, :, None]))[0, :, 0]
                raw_steps[it - 1] = dv
                dv = np.where(dv > max_step, max_step, np.where(dv < -max_step, -max_step, dv))
                pos = pos.copy()
                pos[sel] = pos[sel] + dv
                n_iter, visited[it - 1] = it, pos[sel]
                last_step = steps[it - 1] = np.max(np.abs(dv))
                if np.any(np.abs(pos[sel] - start) > max_offset):
                    status = 5
                    break
                if tol > 0 and last_step < tol:
                    status = 0
                    break
            if status == 4 and tol == 0:
                status = 0
            if status == 0:
                ev = evaluate(pos)
                trace[n_iter] = slots(pos)
                ratio = min(ratio, ev["ratio"])
                if ev["n_cadences"] == 0:
                    status = 1
                else:
                    L2, singular, r2 = factor(ev["H"])
                    ratio = min(ratio, r2)
                    if singular:
                        status = 3
                    else:
                        Minv = _psf_forward(L2, np.eye(P)[None])[0]                # L2^-1
                        cov = Minv.T @ Minv
                        full = slots(pos)
                        out["star_col"], out["star_row"] = np.where(fit, full[0::2], col_in), np.where(fit, full[1::2], rw_in)
                        at = np.stack([2 * fitted_index, 2 * fitted_index + 1], axis=1).reshape(-1)
                        out["position_cov"][np.ix_(at, at)] = cov
                        err = np.sqrt(np.diag(cov))
                        out["star_col_err"][fitted_index], out["star_row_err"][fitted_index] = err[0::2], err[1::2]
                        out["chi2"] = float(ev["chi2"])
        # an empty slot is NaN whether or not fit_star names it
        empty = np.isnan(col_in) | np.isnan(rw_in)
        out["star_col"], out["star_row"] = np.where(empty, np.nan, out["star_col"]), np.where(empty, np.nan, out["star_row"])
        out.update(status=status, n_cadences=ev["n_cadences"], n_pixels=ev["n_pixels"], n_iter=n_iter, last_step=float(last_step),
                   trace=trace, cadence_status=ev["cadence_status"], n_used=n_used, star_index=star_index, fitted_index=fitted_index,
                   steps=steps, raw_steps=raw_steps, visited=visited, start=start, min_pivot_ratio=float(ratio),
                   first_gradient=first["g"], first_hessian=first["H"])
        return out

    def pixel_periodogram(self, frequency, normalization="amplitude", freq_unit=None, oversample_factor=None):
        """One Lomb-Scargle spectrum per pixel on ONE shared ``frequency`` grid, and where each peaks: which pixels vary, and at
        which frequency (what ``TargetPixelFile.plot_pixels(periodogram=True)`` loops for; the host mirror of
        ``DevicePixelCubeBatch.pixel_periodograms`` and its definition, float64 numpy after the float32 load; same keys without
        the batch axis).  Cadences with a non-finite time are dropped for the whole cutout, ``t_ref`` is the first finite time;
        pixel p is taken on the remaining cadences where its own flux is not NaN, ``n_used[p]`` of them, with unit weights
        (``flux_err`` is not read).  Its spectrum is what ``LombScarglePeriodogram.from_lightcurve`` returns for that light
        curve with an exact ``ls_method``: astropy's floating-mean GLS from the exact trigonometric sums, then
        ``normalization`` 'amplitude': ``sqrt(P_psd) * sqrt(4 / n_used)``, ``frequency`` in 1/d by default; 'psd': ``P_psd * 2 /
        (n_used * oversample_factor * fs)`` with ``fs = 1 / (t_last - t_first) / oversample_factor`` in microhertz from the
        pixel's own first and last used time, ``frequency`` in microhertz by default, ``oversample_factor`` 1 by default.
        ``frequency``: F values in ``freq_unit``, each finite and > 0 (``ValueError`` otherwise).  A pixel with ``n_used`` < 4
        has a NaN spectrum; a cutout with fewer than 4 finite times has ``status`` 2, every spectrum NaN and ``n_used`` 0
        (``status`` 0 otherwise).  Returns a dict: ``power`` (F, ny, nx); ``peak_index`` (ny, nx) int32, the first index of the
        largest non-NaN power, -1 without one; ``peak_power`` and ``peak_frequency`` [1/d] (ny, nx), NaN where ``peak_index`` is
        -1; ``n_used`` (ny, nx) int32; ``status``; ``t_ref``; ``frequency`` in 1/d.  Unlike the reference no ``corrector_func``
        runs per pixel (its default removes outliers): clean the cube first, for instance with ``subtract_background``."""
        from ..periodogram import UHZ_PER_CPD, _freq_unit_factor
        if normalization not in ("amplitude", "psd"):
            raise ValueError("normalization must be 'amplitude' or 'psd' (got %r)" % (normalization,))
        unit = freq_unit if freq_unit is not None else ("1/d" if normalization == "amplitude" else "uHz")
        freq = np.atleast_1d(np.asarray(frequency, dtype=np.float64))
        if freq.ndim != 1 or freq.size < 1 or not (np.all(np.isfinite(freq)) and np.all(freq > 0)):
            raise ValueError("frequency must be a 1-D grid of finite values > 0")
        if oversample_factor is None:
            oversample_factor = 5.0 if normalization == "amplitude" else 1.0
        osf = float(oversample_factor)
        if not (osf > 0 and np.isfinite(osf)):
            raise ValueError("oversample_factor must be finite and > 0 (got %r)" % (oversample_factor,))
        f_day = freq / _freq_unit_factor(unit)
        F = len(f_day)
        ny, nx = self.shape[1:]
        fin = np.isfinite(self.time)
        t_ref = float(self.time[fin][0]) if fin.any() else np.nan
        status = 2 if fin.sum() < 4 else 0
        power = np.full((F, ny * nx), np.nan)
        n_used = np.zeros(ny * nx, dtype=np.int32)
        if status == 0:
            t_abs = self.time[fin]
            t = t_abs - t_ref
            y = np.asarray(self.flux, dtype=np.float64)[fin].reshape(len(t), ny * nx)
            with np.errstate(all="ignore"):
                ph = (2 * np.pi * f_day)[None, :] * t[:, None]
                s_all, c_all, s2_all, c2_all = np.sin(ph), np.cos(ph), np.sin(2 * ph), np.cos(2 * ph)
                for p in range(ny * nx):
                    ok = ~np.isnan(y[:, p])
                    n = int(ok.sum())
                    n_used[p] = n
                    if n < 4:
                        continue
                    full = n == len(t)
                    s, c, s2, c2 = (a if full else a[ok] for a in (s_all, c_all, s2_all, c2_all))
                    yp, tp = (y[:, p], t_abs) if full else (y[ok, p], t_abs[ok])
                    w = 1.0 / n
                    yc = yp - (yp[0] + np.sum(yp - yp[0]) * w)
                    Sh, Ch = yc.dot(s) * w, yc.dot(c) * w
                    S, C, S2, C2 = s.sum(axis=0) * w, c.sum(axis=0) * w, s2.sum(axis=0) * w, c2.sum(axis=0) * w
                    tan2 = (S2 - 2 * S * C) / (C2 - (C * C - S * S))
                    C2w = 1 / np.sqrt(1 + tan2 * tan2)
                    S2w = tan2 * C2w
                    Cw = np.sqrt(0.5) * np.sqrt(1 + C2w)
                    Sw = np.sqrt(0.5) * np.sign(S2w) * np.sqrt(1 - C2w)
                    YC, YS = Ch * Cw + Sh * Sw, Sh * Cw - Ch * Sw
                    CC = 0.5 * (1 + C2 * C2w + S2 * S2w) - (C * Cw + S * Sw) ** 2
                    SS = 0.5 * (1 - C2 * C2w - S2 * S2w) - (S * Cw - C * Sw) ** 2
                    psd = (YC * YC / CC + YS * YS / SS) * (0.5 * n)
                    if normalization == "amplitude":
                        power[:, p] = np.sqrt(psd) * np.sqrt(4.0 / n)
                    else:
                        fs = (1.0 / (tp[-1] - tp[0])) / osf * UHZ_PER_CPD
                        power[:, p] = psd * (2.0 / (n * osf * fs))
        has = ~np.isnan(power)
        peak_index = np.where(has.any(axis=0), np.argmax(np.where(has, power, -np.inf), axis=0), -1).astype(np.int32)
        at = np.clip(peak_index, 0, F - 1)
        found = peak_index >= 0
        peak_power = np.where(found, power[at, np.arange(ny * nx)], np.nan)
        peak_frequency = np.where(found, f_day[at], np.nan)
        return {"power": power.reshape(F, ny, nx), "peak_index": peak_index.reshape(ny, nx),
                "peak_power": peak_power.reshape(ny, nx), "peak_frequency": peak_frequency.reshape(ny, nx),
                "n_used": n_used.reshape(ny, nx), "status": status, "t_ref": t_ref, "frequency": f_day}


    def _aperture_sums(self, ap):
        """(flux, flux_err) of the aperture `ap` (boolean image) per cadence, in the cube's dtype.  The gather `cube[:, ap]`
        is kept even for a full aperture: numpy lays its result out pixel-major, so the float32 sums below add the pixels
        of a cadence one after the other — reshaping the cube instead would sum pairwise and round differently (1e-7)."""
        n = len(self.time)
        with np.errstate(all="ignore"):
            pix = self.flux[:, ap]
            perr = self.flux_err[:, ap]
            flux = np.asarray(np.sum(pix, axis=1))
            flux_err = np.sum(perr ** 2, axis=1)
            if pix.shape[1] and np.all(np.isfinite(flux)) and np.all(np.isfinite(flux_err)):
                # every aperture pixel is finite (a NaN / inf would have reached its row's sum): nansum == sum, no cadence
                # is empty, and only a row that sums to zero can be all zeros
                for r in np.flatnonzero(flux == 0):
                    if np.all(self.flux[r] == 0):
                        flux[r] = np.nan
                return flux, flux_err ** 0.5
            flux = np.asarray(np.nansum(pix, axis=1))
            flux[~np.any(np.isfinite(pix), axis=1)] = np.nan
            flux[np.all(self.flux.reshape(n, -1) == 0, axis=1)] = np.nan
            flux_err = np.nansum(perr ** 2, axis=1) ** 0.5
        return flux, flux_err

    def pixel_periodograms(self, frequency=None, corrector="remove_outliers", sigma=5.0, normalization="amplitude",
                           ls_method="fast", device=0, **kwargs):
        """One Lomb-Scargle periodogram per pixel — the loop of ``TargetPixelFile.plot_pixels(periodogram=True)``
        (reference src/lightkurve/targetpixelfile.py:1958-1974: per pixel a one-pixel aperture light curve,
        ``corrector_func`` (default ``remove_outliers``), ``to_periodogram(**kwargs)``) — as batched GPU calls: ONE sigma
        clip over all pixels and ONE periodogram launch per group of pixels that share a frequency grid (all of them when
        ``frequency`` is given; otherwise each pixel's default grid depends on which of its cadences survived the clip).
        Returns a list (row-major over the pixels) of ``LombScarglePeriodogram`` objects, ``None`` where a pixel has no
        usable cadence — the reference's ``pixel_list``."""
        from .. import _capi as capi
        from ..batch import lombscargle_batch
        from ..periodogram import LombScarglePeriodogram, _ls_plan
        n, nr, nc = self.shape
        flux = np.asarray(self.flux, dtype=np.float64).reshape(n, nr * nc)
        ferr = np.asarray(self.flux_err, dtype=np.float64).reshape(n, nr * nc)
        npx = nr * nc
        y = np.ascontiguousarray(flux.T).ravel()                       # pixel-major ragged batch, n cadences each
        off = np.arange(npx + 1, dtype=np.int64) * n
        if corrector == "remove_outliers":
            bad = capi.sigma_clip_batch(y, off, sigma=sigma, device=device).reshape(npx, n)
        elif corrector is None:
            bad = np.zeros((npx, n), bool)
        else:
            raise ValueError("corrector must be 'remove_outliers' or None on the batched path")
        lcs, idx = [], []
        for j in range(npx):
            keep = ~bad[j]
            if not np.any(keep & np.isfinite(flux[:, j])):
                continue
            lcs.append(LightCurve(time=self.time[keep], flux=flux[keep, j], flux_err=ferr[keep, j], meta=dict(self.meta)))
            idx.append(j)
        out = [None] * npx
        # group the pixels by frequency grid (one launch per group)
        groups = {}
        plans = {}
        for lc, j in zip(lcs, idx):
            try:
                plan = _ls_plan(lc, frequency=frequency, normalization=normalization, ls_method=ls_method, **kwargs)
            except IndexError:          # the reference appends None for a light curve too short for a grid
                continue
            plans[j] = plan
            groups.setdefault(plan["frequency"].tobytes(), []).append(j)
        by_pix = dict(zip(idx, lcs))
        for key, members in groups.items():
            p0 = plans[members[0]]
            power = lombscargle_batch([by_pix[j] for j in members], p0["frequency"], normalization=normalization,
                                      freq_unit=p0["freq_unit"], ls_method=ls_method, device=device, gather=False,
                                      oversample_factor=kwargs.get("oversample_factor"), nterms=kwargs.get("nterms", 1))
            for row, j in zip(power, members):
                pl = plans[j]
                out[j] = LombScarglePeriodogram(frequency=pl["frequency"], power=row, nyquist=pl["nyquist"],
                                                default_view=pl["default_view"], ls_method=pl["ls_method"],
                                                nterms=pl["nterms"], meta=pl["lc"].meta,
                                                frequency_unit=pl["freq_unit"], power_unit=pl["power_unit"])
        return out


def _percentile_knots(time, n_knots, degree):
    """[min, interior knots, max] of patsy's bs(x, df=n_knots, degree, include_intercept=True)."""
    order = degree + 1
    n_inner = n_knots - order
    if n_inner < 0:
        raise ValueError("df={} is too small for degree={}; must be >= {}".format(n_knots, degree, order))
    inner = np.percentile(time, np.linspace(0, 100, n_inner + 2)[1:-1]) if n_inner > 0 else np.zeros(0)
    return np.concatenate([[np.min(time)], inner, [np.max(time)]])


def _percentile_knot_plan(n, n_knots, degree):
    """Where ``_percentile_knots`` finds its interior knots in ``n`` NON-DECREASING times: (lo int32[n_inner], g float64[n_inner])
    with knot_k = lerp(t[lo_k], t[min(lo_k + 1, n - 1)], g_k) — np.percentile's 'linear' method (virtual index (n - 1) q,
    numpy/lib/_function_base_impl.py ``_quantile``).  Depends on n and the knot count only: the device gathers and lerps."""
    order = degree + 1
    n_inner = n_knots - order
    if n_inner < 0:
        raise ValueError("df={} is too small for degree={}; must be >= {}".format(n_knots, degree, order))
    q = np.true_divide(np.linspace(0, 100, n_inner + 2)[1:-1], np.float64(100))
    vi = (n - 1) * q
    lo = np.floor(vi)
    above = vi >= n - 1
    lo[above] = n - 1
    g = vi - lo
    g[above] = 0.0
    return lo.astype(np.int32), np.ascontiguousarray(g, dtype=np.float64)


def _knots_from_plan(time, lo, g):
    """[t[0], numpy's _lerp(t[lo], t[lo + 1], g) ..., t[-1]]: the arithmetic of the device's knot gather, in numpy."""
    time = np.asarray(time, dtype=np.float64)
    a, b = time[lo], time[np.minimum(lo + 1, len(time) - 1)]
    d = b - a
    inner = np.where(g >= 0.5, b - d * (1 - g), a + d * g)
    return np.concatenate([[time[0]], inner, [time[-1]]])


def _sequential_aperture_sums(flux, flux_err, ap):
    """``PixelCube._aperture_sums`` for float32 cubes written as the loop the device runs (``cube_aperture_kernel``): per
    cadence the aperture's pixels one after the other in row-major order in float32, NaN pixels (and NaN e * e) skipped,
    flux NaN where no aperture pixel is finite or the whole image is 0, flux_err = sqrt(sum(e * e))."""
    flux, flux_err = np.asarray(flux, dtype=np.float32), np.asarray(flux_err, dtype=np.float32)
    n = flux.shape[0]
    f2, e2 = flux.reshape(n, -1), flux_err.reshape(n, -1)
    acc_f, acc_e = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    anyfinite = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for p in np.flatnonzero(np.asarray(ap, dtype=bool).reshape(-1)):
            v = f2[:, p]
            acc_f = np.where(np.isnan(v), acc_f, acc_f + v).astype(np.float32)
            anyfinite |= np.isfinite(v)
            sq = (e2[:, p] * e2[:, p]).astype(np.float32)
            acc_e = np.where(np.isnan(sq), acc_e, acc_e + sq).astype(np.float32)
        acc_f[~anyfinite | np.all(f2 == 0, axis=1)] = np.nan
        return acc_f, np.sqrt(acc_e)


def _finite_columns(cube2d):
    return cube2d[:, np.all(np.isfinite(cube2d), axis=0)]


class PLDCorrector(RegressionCorrector):
    def __init__(self, tpf, aperture_mask=None):
        if aperture_mask is None:
            aperture_mask = tpf.create_threshold_mask(3)
        self.aperture_mask = tpf._parse_aperture_mask(aperture_mask)
        lc = tpf.to_lightcurve(aperture_mask=self.aperture_mask)
        nan_mask = np.isnan(lc.flux) | np.isnan(lc.flux_err)
        f32 = lc._flux_f32[~nan_mask]
        lc = lc[~nan_mask]
        lc._flux_f32 = f32
        self.tpf = tpf[~nan_mask]
        super().__init__(lc=lc)

    def __repr__(self):
        return "PLDCorrector (ID: {})".format(self.lc.label)

    def _resolve(self, pld_order, pca_components, pld_aperture_mask, normalize_background_pixels):
        """mission defaults of .correct() (pldcorrector.py:382-403)."""
        k2 = self.tpf.meta.get("MISSION") == "K2"
        if pld_order is None:
            pld_order = 3 if k2 else 1
        if pca_components is None:
            pca_components = 16 if k2 else 3
        if pld_aperture_mask is None:
            pld_aperture_mask = "threshold" if k2 else "empty"
        if normalize_background_pixels is None:
            normalize_background_pixels = bool(k2)
        return pld_order, pca_components, pld_aperture_mask, normalize_background_pixels

    def create_design_matrix(self, pld_order=3, pca_components=16, pld_aperture_mask=None,
                             background_aperture_mask="background", spline_n_knots=None, spline_degree=3,
                             normalize_background_pixels=None, sparse=False, device=0):
        """DesignMatrixCollection [pixel_series | background | spline] built on the GPU (one cutout = a batch of 1)."""
        if pca_components is None or pca_components < 1:
            raise NotImplementedError("pca_components must be >= 1 on the HIP path")
        # None -> all pixels, exactly as the reference's create_design_matrix treats it (pldcorrector.py:203-207;
        # correct() resolves the mission-dependent default before it calls this)
        self.pld_aperture_mask = self.tpf._parse_aperture_mask(pld_aperture_mask)
        self.background_aperture_mask = self.tpf._parse_aperture_mask(background_aperture_mask)
        n = len(self.lc)
        if spline_n_knots is None:
            spline_n_knots = int(n / 50)
        if normalize_background_pixels is None:
            normalize_background_pixels = False
        cube = self.tpf.flux
        pld_pix = _finite_columns(cube[:, self.pld_aperture_mask].reshape(n, -1))
        bkg_pix = _finite_columns(cube[:, self.background_aperture_mask].reshape(n, -1))
        knots = _percentile_knots(self.lc.time, spline_n_knots, spline_degree)
        X, ps = _capi.pld_design_batch(pld_pix[None] if pld_pix.shape[1] else None, bkg_pix[None],
                                       self.lc._flux_f32[None], self.lc.time[None], knots[None], pld_order,
                                       pca_components, spline_degree, normalize_background_pixels, device=device)
        X, ps = X[0], ps[0]
        nsp = spline_n_knots + 1
        kb = min(pca_components, bkg_pix.shape[1])
        npld = X.shape[1] - nsp - kb
        mats = []
        if npld > 0:
            mats.append(DesignMatrix(X[:, :npld], name="pixel_series", prior_sigma=ps[:npld]))
        mats.append(DesignMatrix(X[:, npld:npld + kb], name="background", prior_sigma=ps[npld:npld + kb]))
        if sparse:
            # reference :194-199, 226-230: the sparse collection carries a DIFFERENT spline basis
            # (create_sparse_spline_matrix); pixel and background blocks are the same PCA'd matrices
            sp = create_sparse_spline_matrix(self.lc.time, n_knots=spline_n_knots, degree=spline_degree).append_constant()
            sp.prior_sigma = np.ones(sp.shape[1]) * ps[-1]
            mats.append(sp)
            return SparseDesignMatrixCollection(mats)
        mats.append(DesignMatrix(X[:, npld + kb:], name="spline", prior_sigma=ps[npld + kb:],
                                 columns=["knot{}".format(i + 1) for i in range(spline_n_knots)] + ["offset"]))
        return DesignMatrixCollection(mats)

    def correct(self, pld_order=None, pca_components=None, pld_aperture_mask=None,
                background_aperture_mask="background", spline_n_knots=None, spline_degree=5,
                normalize_background_pixels=None, restore_trend=True, sparse=False, cadence_mask=None, sigma=5,
                niters=5, propagate_errors=False, device=0):
        """Same contract and defaults as the reference (pldcorrector.py:304-427)."""
        self.restore_trend = restore_trend
        pld_order, pca_components, pld_aperture_mask, normalize_background_pixels = self._resolve(
            pld_order, pca_components, pld_aperture_mask, normalize_background_pixels)
        dm = self.create_design_matrix(pld_aperture_mask=pld_aperture_mask,
                                       background_aperture_mask=background_aperture_mask, pld_order=pld_order,
                                       pca_components=pca_components, spline_n_knots=spline_n_knots,
                                       spline_degree=spline_degree,
                                       normalize_background_pixels=normalize_background_pixels, sparse=sparse,
                                       device=device)
        clc = super().correct(dm, cadence_mask=cadence_mask, sigma=sigma, niters=niters,
                              propagate_errors=propagate_errors, device=device)
        if restore_trend:
            sp = self.diagnostic_lightcurves["spline"].flux
            clc.flux = clc.flux + (sp - np.median(sp))
        return clc


def _all_finite(a):
    """np.all(np.isfinite(a)) without the boolean temporary in the common case: a finite float64 total implies it."""
    with np.errstate(all="ignore"):
        return bool(np.isfinite(a.sum(dtype=np.float64))) or bool(np.all(np.isfinite(a)))


def _shared_mask(first, spec, sap=False):
    """A mask every cutout of the batch shares — given as an array, or by a name that depends on the cutout's SHAPE only
    ('all', 'empty'; None = all pixels for the PLD / background masks) — as a boolean image; None for the specs the reference
    evaluates on each target-pixel file's own DATA ('threshold', 'background'; None for the photometric aperture =
    ``create_threshold_mask(3)``, pldcorrector.py:99-107): those are resolved per cutout in ``_batch_cutout``."""
    if spec is None:
        return None if sap else first._parse_aperture_mask(None)
    if isinstance(spec, str) and spec in ("threshold", "background"):
        return None
    return first._parse_aperture_mask(spec)


def _per_cutout_masks(spec, B, image_shape):
    """A mask argument given as a bool (B, ny, nx) array — one mask per cutout — or None for every other kind of spec."""
    if spec is None or isinstance(spec, str):
        return None
    m = np.asarray(spec, dtype=bool)
    if m.ndim != 3:
        return None
    if m.shape != (B,) + tuple(image_shape):
        raise ValueError("per-cutout masks have shape {}, but the batch holds {} cutouts of shape {}".format(
            m.shape, B, tuple(image_shape)))
    return m


def _ragged_index_lists(masks, pca_components, what="PLD"):
    """bool (B, npix) masks of DIFFERENT sizes -> (idx int32 (B, Pmax): every cutout's selected pixel numbers ascending, then -1;
    counts int32 (B,)) — the layout ``lk_pld_gather_ragged_batch_dev`` reads.  Every count must reach ``pca_components``: the PCA
    keeps min(pca_components, count) columns, so a smaller block would give that cutout a narrower design matrix than the rest
    of the call.  ValueError names the cutouts and their counts."""
    masks = np.asarray(masks, dtype=bool)
    if masks.ndim != 2 or masks.shape[0] < 1:
        raise ValueError("masks must be (B, npix)")
    counts = masks.sum(axis=1).astype(np.int32)
    short = np.flatnonzero(counts < int(pca_components))
    if short.size:
        raise ValueError("ragged_masks: the %s masks of cutouts %s select %s pixels, fewer than pca_components = %d; correct these "
                         "cutouts on their own or lower pca_components"
                         % (what, short.tolist(), counts[short].tolist(), int(pca_components)))
    idx = np.full((masks.shape[0], max(int(counts.max()), 1)), -1, dtype=np.int32)
    for b, m in enumerate(masks):
        idx[b, :counts[b]] = np.flatnonzero(m)
    return idx, counts


def _batch_cutout(c, ap, pm, bm, specs):
    """One cutout's share of pld_correct_batch: what ``PLDCorrector(c, aperture_mask)`` keeps (the SAP light curve without its
    NaN cadences, pldcorrector.py:109-120) and the pixel series of the two apertures, without the object construction.
    ``ap`` / ``pm`` / ``bm``: shared boolean images, or None = evaluate ``specs`` (aperture, PLD, background) on THIS cutout as
    the per-object corrector does — the photometric aperture on the whole cutout (``PLDCorrector.__init__``), the other
    two on the cutout without its NaN cadences (``create_design_matrix`` sees ``self.tpf = tpf[~nan_mask]``).
    Returns (time, flux float64, flux_err float64, flux float32, pld pixels (n, P), background pixels (n, Pb))."""
    if ap is None:
        ap = c._parse_aperture_mask(c.create_threshold_mask(3) if specs[0] is None else specs[0])
    flux, ferr = c._aperture_sums(ap)
    keep = ~(np.isnan(flux) | np.isnan(ferr))
    everything = bool(keep.all())
    n_all = len(c.time)
    if pm is None or bm is None:
        ck = c if everything else c[keep]
        pm = ck._parse_aperture_mask(specs[1]) if pm is None else pm
        bm = ck._parse_aperture_mask(specs[2]) if bm is None else bm

    def pixels(mask):
        px = c.flux.reshape(n_all, -1) if bool(np.all(mask)) else c.flux[:, mask]
        return px if everything else px[keep]

    pld = pixels(pm)
    bkg = pld if (pm.shape == bm.shape and np.array_equal(pm, bm)) else pixels(bm)
    if not everything:
        flux, ferr = flux[keep], ferr[keep]
    return (c.time if everything else c.time[keep], np.asarray(flux, dtype=np.float64), np.asarray(ferr, dtype=np.float64),
            np.asarray(flux, dtype=np.float32), pld, bkg)


def pld_correct_batch(cubes, aperture_mask="all", pld_aperture_mask="all", background_aperture_mask="all",
                      pld_order=3, pca_components=16, spline_n_knots=None, spline_degree=5,
                      normalize_background_pixels=True, restore_trend=True, sigma=5, niters=5, device=0, ragged_masks=False):
    """PLDCorrector(...).correct(...) for a list of same-shaped cutouts in ONE GPU call (``lk_pld_correct_batch``: design
    matrices, regression and the spline block's share of the model; the design matrices never leave the device).  Masks
    given as arrays (or 'all' / 'empty') are shared by the batch; the data-dependent ones — ``aperture_mask=None`` (the
    reference's default, ``create_threshold_mask(3)``), 'threshold', 'background' — are evaluated on EVERY cutout, as a loop
    over ``PLDCorrector(tpf, aperture_mask).correct(...)`` would (pldcorrector.py:99-107, 203-207); such PLD / background
    masks must then select the same NUMBER of pixels in every cutout (one design-matrix width per call) unless
    ``ragged_masks=True``: then the pixel blocks are zero-padded to the widest cutout's and go with their per-cutout counts to
    ``lk_pld_correct_ragged_batch`` (every count >= ``pca_components``; equal sizes take the call without the keyword).  Each
    mask may also be a bool (B, ny, nx) array, one mask per cutout.  The per-cutout host
    work (aperture sums, NaN-cadence removal, pixel gathers, percentile knots) runs on the packing thread pool and lands in
    page-locked staging buffers.  Returns (corrected_flux[B, N], outlier_mask[B, N])."""
    from .. import packed
    cubes = list(cubes)
    if not cubes:
        raise ValueError("pld_correct_batch needs at least one cutout")
    if pca_components is None or pca_components < 1:
        raise NotImplementedError("pca_components must be >= 1 on the HIP path")
    first = cubes[0]
    specs = (aperture_mask, pld_aperture_mask, background_aperture_mask)
    per = [_per_cutout_masks(spec, len(cubes), first.shape[1:]) for spec in specs]
    ap = None if per[0] is not None else _shared_mask(first, aperture_mask, sap=True)
    pm = None if per[1] is not None else _shared_mask(first, pld_aperture_mask)
    bm = None if per[2] is not None else _shared_mask(first, background_aperture_mask)
    for c in cubes:
        if c.shape[1:] != first.shape[1:]:
            raise ValueError("pld_correct_batch needs cutouts of one shape (got %s and %s)" % (c.shape, first.shape))

    def own(i, shared_mask, b):
        return per[i][b] if per[i] is not None else shared_mask

    parts = packed._pmap(_batch_cutout, [(c, own(0, ap, b), own(1, pm, b), own(2, bm, b), specs) for b, c in enumerate(cubes)])
    n = len(parts[0][0])
    if any(len(p[0]) != n for p in parts):
        raise ValueError("pld_correct_batch needs cutouts with the same number of valid cadences")
    B = len(parts)
    counts_p = np.array([p[4].shape[1] for p in parts], dtype=np.int32)
    counts_b = np.array([p[5].shape[1] for p in parts], dtype=np.int32)
    P, Pb = int(counts_p.max()), int(counts_b.max())         # (ragged: the row pitch of the zero-padded blocks)
    ragged = bool(np.any(counts_p != P) or np.any(counts_b != Pb))
    if ragged and ragged_masks:
        for counts, what in ((counts_p, "PLD"), (counts_b, "background")):
            short = np.flatnonzero(counts < int(pca_components))
            if short.size and counts.max() > 0:
                raise ValueError("ragged_masks: the %s masks of cutouts %s select %s pixels, fewer than pca_components = %d; "
                                 "correct these cutouts on their own or lower pca_components"
                                 % (what, short.tolist(), counts[short].tolist(), int(pca_components)))
    elif ragged:
        raise ValueError("pld_correct_batch: the per-cutout '%s' / '%s' masks select different numbers of pixels (%s PLD, %s "
                         "background); pass masks of one size or correct these cutouts one by one"
                         % (pld_aperture_mask, background_aperture_mask, sorted({p[4].shape[1] for p in parts}),
                            sorted({p[5].shape[1] for p in parts})))
    shared = all(p[5] is p[4] for p in parts)
    if spline_n_knots is None:
        spline_n_knots = int(n / 50)

    def staged(key, shape, dtype):
        count = int(np.prod(shape))
        try:
            return _capi.pinned_pool("pld_" + key, count, dtype).reshape(shape)
        except (OSError, RuntimeError, MemoryError):
            return np.empty(shape, dtype=dtype)

    pld = staged("pix", (B, n, P), np.float32)
    bkg = pld if shared else staged("bkg", (B, n, Pb), np.float32)
    lcf = staged("lcf", (B, n), np.float32)
    t, y, err = (staged(k, (B, n), np.float64) for k in ("t", "y", "err"))
    knots = np.empty((B, max(spline_n_knots - spline_degree - 1, 0) + 2), dtype=np.float64)

    def fill(b):
        tb, fb, eb, f32, px, bx = parts[b]
        t[b], y[b], err[b], lcf[b] = tb, fb, eb, f32
        pld[b, :, :px.shape[1]] = px
        pld[b, :, px.shape[1]:] = 0.0
        if not shared:
            bkg[b, :, :bx.shape[1]] = bx
            bkg[b, :, bx.shape[1]:] = 0.0
        knots[b] = _percentile_knots(tb, spline_n_knots, spline_degree)
        return _all_finite(px) and (shared or _all_finite(bx))

    if not all(packed._pmap(fill, [(b,) for b in range(B)])):
        raise ValueError("pld_correct_batch needs finite pixels inside the masks")
    res = _capi.pld_correct_batch(pld if P else None, bkg, lcf, t, knots, y, err, pld_order, pca_components, spline_degree,
                                  normalize_background_pixels, sigma=sigma, niters=niters, want_spline=restore_trend,
                                  device=device, p_count=counts_p if ragged and P else None,
                                  pb_count=counts_b if ragged else None)
    corrected = y - res["model"]
    if restore_trend:
        sp = res["spline"]
        corrected += sp - np.median(sp, axis=1)[:, None]
    return corrected, res["outlier_mask"]
