"""Device-resident batch of target-pixel cutouts: ``DevicePixelCubeBatch`` (aperture photometry, centroids, background,
difference / amplitude images, pixel periodograms, PSF photometry and PLD on cubes that went up once), the checks of its
inputs and the call scaffolding its methods share — mask staging, per-cutout arguments, image centroids, downloads.
device.py re-exports the class; the light-curve classes are imported inside the methods that return them."""
import ctypes

import numpy as np

from . import _capi
from . import packed
from .devmem import DeviceBuffer, _dp, _i32p, _off_ptr, _p, _upload, _vp


def _per_cutout(name, a, B, finite=True):
    """``a``, a scalar or one value per cutout -> C-contiguous float64 (B,)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.size != B):
        raise ValueError("%s must be a scalar or one value per cutout (%d), got shape %r" % (name, B, a.shape))
    if finite and not np.all(np.isfinite(a)):
        raise ValueError("%s must be finite" % name)
    return np.ascontiguousarray(np.broadcast_to(a, (B,)))


def _first_finite_times(time):
    """``t_ref`` of the per-pixel fits: each row's first finite time of the host (B, N) array, NaN for a row without one."""
    fin = np.isfinite(time)
    return np.ascontiguousarray(np.where(fin.any(axis=1), time[np.arange(len(time)), np.argmax(fin, axis=1)], np.nan))


def _psf_stars(B, star_col, star_row, sigma):
    """The stars and widths of the PSF calls, checked -> ((star_col, star_row) as C-contiguous float64 [B, S_max], the bool [B,
    S_max] of the stars that take part (no NaN coordinate), sigma float64 [B, 2] (None for ``sigma`` None: a call with a
    tabulated PRF), S_max)."""
    from .correctors.pldcorrector import _psf_sigma
    pos = []
    for name, a in (("star_col", star_col), ("star_row", star_row)):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = np.broadcast_to(a, (B, a.size))
        if a.ndim != 2 or a.shape[0] != B:
            raise ValueError("%s must be [S] or [B, S] with B = %d (got shape %r)" % (name, B, a.shape))
        pos.append(np.ascontiguousarray(a))
    if pos[0].shape != pos[1].shape or not 1 <= pos[0].shape[1] <= 8:
        raise ValueError("star_col and star_row must have one shape with 1 .. 8 stars per cutout (got %r and %r)"
                         % (pos[0].shape, pos[1].shape))
    part = ~(np.isnan(pos[0]) | np.isnan(pos[1]))
    if not np.all(np.isfinite(pos[0][part]) & np.isfinite(pos[1][part])):
        raise ValueError("a star position is infinite")
    if not np.all(part.any(axis=1)):
        raise ValueError("cutouts %s have no star" % np.flatnonzero(~part.any(axis=1)).tolist())
    if sigma is None:
        return pos, part, None, pos[0].shape[1]
    sg = np.asarray(sigma, dtype=np.float64)
    sg = np.array([_psf_sigma(s) for s in sg]) if sg.shape == (B, 2) else np.tile(_psf_sigma(sg), (B, 1))
    return pos, part, np.ascontiguousarray(sg, dtype=np.float64), pos[0].shape[1]


def _prf_index(what, B, sigma, prf, prf_index):
    """The ``prf`` / ``prf_index`` checks of ``psf_photometry`` and ``psf_fit`` -> the table of every cutout, int32 [B], or None
    without ``prf``."""
    from .correctors.pldcorrector import TabulatedPRF
    if (sigma is None) == (prf is None):
        raise ValueError("%s takes exactly one of sigma and prf" % what)
    if prf is None:
        if prf_index is not None:
            raise ValueError("prf_index needs prf")
        return None
    if not isinstance(prf, TabulatedPRF):
        raise ValueError("prf must be a TabulatedPRF (got %r)" % (type(prf),))
    pidx = np.zeros(B, dtype=np.int32) if prf_index is None else np.asarray(prf_index)
    if pidx.ndim > 1 or (pidx.ndim == 1 and pidx.size != B) or pidx.dtype.kind not in "iu":
        raise ValueError("prf_index must be an integer or one integer per cutout (%d)" % B)
    if np.any(pidx < 0) or np.any(pidx >= prf.n_prf):
        raise ValueError("prf_index must be 0 .. %d" % (prf.n_prf - 1))
    return np.ascontiguousarray(np.broadcast_to(pidx, (B,)), dtype=np.int32)


def _prf_device_table(prf, handle, stream):
    """``prf.samples`` in HBM: uploaded once per handle and kept on the ``TabulatedPRF`` (synchronised, so that later calls on
    any stream of the handle may read it)."""
    cache = prf.__dict__.setdefault("_device", {})
    hit = cache.get(handle.device)
    if hit is None or hit[0] is not handle:
        buf, _ = _upload(handle, prf.samples, stream, np.float32)
        _capi._check(_capi._lib.lk_stream_synchronize(handle._h, _vp(stream or None)))
        hit = cache[handle.device] = (handle, buf)
    return hit[1]


# ``info`` of the PSF calls: (key, dtype), B x N values each but ``status`` (B)
_PSF_INFO = (("background", np.float64), ("chi2", np.float64), ("n_used", np.int32), ("cadence_status", np.int8), ("status", np.int32))
_PSF_FIT_INFO = _PSF_INFO + (("shift_col", np.float64), ("shift_row", np.float64), ("shift_col_err", np.float64),
                             ("shift_row_err", np.float64), ("last_step", np.float64), ("n_iter", np.int32))


def _psf_info_spec(B, N, spec):
    """(key, dtype, bytes) of every ``info`` buffer of a PSF call."""
    return [(key, dt, (B if key == "status" else B * N) * np.dtype(dt).itemsize) for key, dt in spec]


def _psf_width_spec(B, N, max_iter):
    """(key, dtype, shape) of every output of ``psf_width``."""
    return [("sigma", np.float64, (B, 2)), ("sigma_err", np.float64, (B, 2)), ("sigma_cov", np.float64, (B,)),
            ("chi2", np.float64, (B,)), ("last_step", np.float64, (B,)), ("trace", np.float64, (B, max_iter + 1, 2)),
            ("n_iter", np.int32, (B,)), ("n_cadences", np.int32, (B,)), ("n_pixels", np.int64, (B,)),
            ("cadence_status", np.int8, (B, N)), ("status", np.int32, (B,))]


def _psf_positions_spec(B, N, S_max, max_iter):
    """(key, dtype, shape) of every output of ``psf_positions``."""
    return [("star_col", np.float64, (B, S_max)), ("star_row", np.float64, (B, S_max)), ("star_col_err", np.float64, (B, S_max)),
            ("star_row_err", np.float64, (B, S_max)), ("position_cov", np.float64, (B, 2 * S_max, 2 * S_max)),
            ("chi2", np.float64, (B,)), ("last_step", np.float64, (B,)), ("trace", np.float64, (B, max_iter + 1, 2 * S_max)),
            ("n_iter", np.int32, (B,)), ("n_cadences", np.int32, (B,)), ("n_pixels", np.int64, (B,)),
            ("cadence_status", np.int8, (B, N)), ("status", np.int32, (B,))]


class DevicePixelCubeBatch(object):
    """B same-shaped target-pixel cutouts IN HBM — the input of ``PLDCorrector`` as ``DeviceLightCurveBatch`` is the input of
    the light-curve chain: ``d_flux`` / ``d_flux_err`` float32 [B][N][npix] (npix = ny * nx, row-major pixels: the layout
    ``lk_fits_unpack_cube`` writes per column), ``d_time`` float64 [B][N], all on ONE stream of the process's handle.
    ``pld_correct_batch`` does, per cutout and on the host: aperture sums, NaN-cadence removal, pixel gathers, percentile
    knots, packing, upload.  Here the cubes go up once and ``lk_cube_aperture_batch_dev`` -> ``lk_pld_gather_batch_dev`` ->
    ``lk_pld_correct_batch_dev`` run on them; the results are the same bits (the same PLD kernels see the same numbers).

        cubes = DevicePixelCubeBatch.from_cubes(list_of_PixelCube)        # or .from_fits(paths) / .from_arrays(t, flux, err)
        corrected, outliers = cubes.pld_correct(pld_order=3, pca_components=16)
        lcs, d_outl = cubes.pld_correct(to_host=False)                    # DeviceLightCurveBatch: .flatten(...) ... follow

    float32 cubes only; every cutout of a call must keep the same number of cadences; ``pld_correct`` needs times that are
    finite and non-decreasing per cutout (the knots are gathered from sorted times) — ``pld_correct_batch`` takes what does
    not fit."""

    def __init__(self, d_time, d_flux, d_flux_err, time, shape, meta=None, device=0, stream=0, is_sorted=None):
        self.handle = _capi.Handle.get(device)
        self.device = int(device)
        self.stream = int(stream or 0)
        self.d_time, self.d_flux, self.d_flux_err = d_time, d_flux, d_flux_err
        self.shape = tuple(int(v) for v in shape)                   # (B, N, ny, nx)
        B, N, ny, nx = self.shape
        if d_time.capacity < B * N * 8 or d_flux.capacity < B * N * ny * nx * 4 or d_flux_err.capacity < B * N * ny * nx * 4:
            raise ValueError("device buffer smaller than the batch it is said to hold")
        self.time = np.ascontiguousarray(time, dtype=np.float64).reshape(B, N)      # host copy (B x N doubles)
        # checked here, on the host's copy; raised by pld_correct — a file whose kept cadences lack a TIME (read as 0.0 like
        # TargetPixelFile.time does) still round-trips and still has aperture photometry
        # (is_sorted: what a batch that shares its parent's times already knows)
        self.is_sorted = _cube_times_sorted(self.time) if is_sorted is None else bool(is_sorted)
        self.meta = list(meta) if meta is not None else [{} for _ in range(B)]
        self._keep = []                                              # host staging the stream may still be reading

    # ---------------------------------------------------------------- construction
    @classmethod
    def from_arrays(cls, time, flux, flux_err, meta=None, device=0, stream=0):
        """H2D once: time[B, N], flux / flux_err [B, N, ny, nx] float32 (page-locked arrays go by DMA)."""
        time, flux, flux_err = _check_cube_arrays(time, flux, flux_err)
        h = _capi.Handle.get(device)
        bufs, keep = [], []
        for a, dt in ((time, np.float64), (flux, np.float32), (flux_err, np.float32)):
            b, k = _upload(h, a, stream, dt)
            bufs.append(b), keep.append(k)
        out = cls(bufs[0], bufs[1], bufs[2], time, flux.shape, meta, device, stream)
        out._keep = keep
        return out

    @classmethod
    def from_cubes(cls, cubes, device=0, stream=0):
        """From a list of ``PixelCube`` of one (N, ny, nx): one packing pass into the page-locked pool, one upload per column."""
        cubes = list(cubes)
        if not cubes:
            raise ValueError("DevicePixelCubeBatch needs at least one cutout")
        shape = cubes[0].shape
        for c in cubes:
            if c.flux.dtype != np.float32 or c.flux_err.dtype != np.float32:
                raise TypeError("DevicePixelCubeBatch holds float32 cubes (got %s / %s); pld_correct_batch takes the others"
                                % (c.flux.dtype, c.flux_err.dtype))
            if c.shape != shape:
                raise ValueError("DevicePixelCubeBatch needs cutouts of one shape (got %s and %s)" % (c.shape, shape))
        B = len(cubes)

        def staged(key, shp, dtype):
            try:
                return _capi.pinned_pool("devcube:" + key, int(np.prod(shp)), dtype).reshape(shp)
            except (OSError, RuntimeError, MemoryError):
                return np.empty(shp, dtype=dtype)

        t = staged("t", (B, shape[0]), np.float64)
        f, e = staged("f", (B,) + shape, np.float32), staged("e", (B,) + shape, np.float32)

        def fill(b):
            t[b], f[b], e[b] = cubes[b].time, cubes[b].flux, cubes[b].flux_err

        packed._pmap(fill, [(b,) for b in range(B)])
        out = cls.from_arrays(t, f, e, [dict(c.meta) for c in cubes], device, stream)
        out.synchronize()              # the staging pool is reused by the next packing call
        out.time = out.time.copy()
        return out

    @classmethod
    def from_fits(cls, paths, quality_bitmask="default", device=0, stream=0):
        """Target-pixel files of one shape and one number of kept cadences -> a resident batch (``PixelCube.from_fits``
        without the way back: headers on the host, ``lk_fits_unpack_cube_dev`` per file in HBM, then a device-to-device
        copy into that file's slice of the batch — the unpacker lays its columns out for the file's OWN row count, which is
        only known to equal the batch's once its cadence selection has run)."""
        from . import fitsio
        paths = list(paths)
        if not paths:
            raise ValueError("DevicePixelCubeBatch needs at least one file")
        h = _capi.Handle.get(device)
        st = _vp(stream or None)
        lib = _capi._lib
        bufs, shape, meta = None, None, []
        for b, path in enumerate(paths):
            tab = fitsio.read_fits_table(path, ext=1)
            pc = fitsio.pixel_columns(tab, columns=("flux", "flux_err"), quality_bitmask=quality_bitmask)
            if pc["columns"] != ["flux", "flux_err"]:
                raise ValueError("%s has no FLUX_ERR column" % path)
            raw = np.ascontiguousarray(tab.raw, dtype=np.uint8)
            n_rows, row_bytes = raw.shape
            npix = int(pc["npix"])
            d_raw = DeviceBuffer(h, raw.nbytes + 16)
            d_raw.upload(raw.reshape(-1), stream)
            d_t, d_q = DeviceBuffer(h, (n_rows + 1) * 8), DeviceBuffer(h, (n_rows + 2) * 4)
            d_c = DeviceBuffer(h, (2 * n_rows * npix + 4) * 4)
            cols = np.ascontiguousarray(pc["col_offsets"], dtype=np.int32)
            kept = np.zeros(1, dtype=np.int64)
            _capi._check(lib.lk_fits_unpack_cube_dev(
                h._h, _p(d_raw), int(row_bytes), int(n_rows), int(pc["off_time"]), int(pc["code_time"]),
                int(pc["off_quality"]), int(pc["code_quality"]), ctypes.c_int64(int(pc["bitmask"])), int(bool(pc["keep_nan_time"])),
                2, cols.ctypes.data_as(_i32p), npix, _p(d_t), _p(d_q), _p(d_c), _off_ptr(kept), st))
            N = int(kept[0])
            cube_shape = (N,) + tuple(int(v) for v in pc["shape"])
            if len(cube_shape) != 3:
                raise ValueError("%s: the pixel columns are not images" % path)
            if bufs is None:
                if N < 2:
                    raise ValueError("%s keeps %d cadences" % (path, N))
                shape = cube_shape
                B = len(paths)
                bufs = (DeviceBuffer(h, B * N * 8), DeviceBuffer(h, B * N * npix * 4), DeviceBuffer(h, B * N * npix * 4))
            elif cube_shape[1:] != shape[1:]:
                raise ValueError("DevicePixelCubeBatch needs cutouts of one shape (got %s and %s)" % (cube_shape, shape))
            elif N != shape[0]:
                raise ValueError("DevicePixelCubeBatch.from_fits needs files that keep the same number of cadences "
                                 "(%s keeps %d, %s keeps %d)" % (path, N, paths[0], shape[0]))
            for dst, src, nbytes in ((bufs[0].ptr + b * N * 8, d_t.ptr, N * 8),
                                     (bufs[1].ptr + b * N * npix * 4, d_c.ptr, N * npix * 4),
                                     (bufs[2].ptr + b * N * npix * 4, d_c.ptr + n_rows * npix * 4, N * npix * 4)):
                _capi._check(lib.lk_memcpy_d2d(h._h, _vp(dst), _vp(src), nbytes, st))
            meta.append({"MISSION": tab.primary.get("MISSION", tab.primary.get("TELESCOP")),
                         "TARGETID": tab.primary.get("KEPLERID", tab.primary.get("TICID")), "FILENAME": str(path),
                         "QUALITY_BITMASK": quality_bitmask, "LABEL": tab.primary.get("OBJECT")})
        B, N = len(paths), shape[0]
        time = bufs[0].download(np.float64, B * N, stream=stream)       # (synchronises; the per-file buffers may go)
        return cls(bufs[0], bufs[1], bufs[2], time, (B,) + shape, meta, device, stream)

    # ---------------------------------------------------------------- plumbing
    def __len__(self):
        return self.shape[0]

    def synchronize(self):
        _capi._check(_capi._lib.lk_stream_synchronize(self.handle._h, _vp(self.stream or None)))
        self._keep = []

    def _get(self, buf, dtype, shape):
        """``buf``'s first prod(shape) elements of ``dtype`` -> host array of ``shape`` (synchronises the batch's stream)."""
        out = np.empty(shape, dtype=dtype)
        return buf.download(dtype, out.size, out=out, stream=self.stream)

    def to_host(self):
        """D2H of the cubes -> list of ``PixelCube`` (round trip, for tests)."""
        from .correctors.pldcorrector import PixelCube
        B, N = self.shape[:2]
        f, e = self._get(self.d_flux, np.float32, self.shape), self._get(self.d_flux_err, np.float32, self.shape)
        t = self._get(self.d_time, np.float64, (B, N))
        self._keep = []
        out = []
        for b in range(B):
            c = PixelCube(t[b], f[b], e[b])
            c.meta.update(self.meta[b])
            out.append(c)
        return out

    # ---------------------------------------------------------------- masks
    def _shape_mask(self, spec, sap):
        """A mask spec that does not depend on the pixels' values -> bool (ny, nx); None for the data-dependent ones
        ('threshold', 'background', and None for the photometric aperture = create_threshold_mask(3))."""
        ny, nx = self.shape[2:]
        if spec is None:
            return None if sap else np.ones((ny, nx), dtype=bool)
        if isinstance(spec, str):
            if spec == "all":
                return np.ones((ny, nx), dtype=bool)
            if spec == "empty":
                return np.zeros((ny, nx), dtype=bool)
            if spec in ("threshold", "background"):
                return None
            raise ValueError("aperture_mask '{}' is not supported here".format(spec))
        m = np.asarray(spec, dtype=bool)
        if m.shape == (self.shape[0], ny, nx):          # one mask per cutout
            return m
        if m.shape != (ny, nx):
            raise ValueError("`aperture_mask` has shape {}, but the flux data has shape {}".format(m.shape, (ny, nx)))
        return m

    def _median_images_dev(self, d_keep=None):
        B, N, ny, nx = self.shape
        d_med = DeviceBuffer(self.handle, B * ny * nx * 8)
        _capi._check(_capi._lib.lk_cube_median_image_batch_dev(self.handle._h, B, N, ny * nx, _p(self.d_flux), _p(d_keep), _p(d_med),
                                                               _vp(self.stream or None)))
        return d_med

    def median_images(self, d_keep=None):
        """np.nanmedian(flux.astype(float64), axis=0) of every cutout, computed on the device (``lk_cube_median_image_batch_dev``)
        over all cadences or those flagged in ``d_keep`` (DeviceBuffer of B x N bytes) -> float64[B, ny, nx] on the host."""
        B, N, ny, nx = self.shape
        return self._get(self._median_images_dev(d_keep), np.float64, (B, ny, nx))

    def threshold_masks(self, threshold=3, reference_pixel="center", d_keep=None, to_host=True, invert=False, _d_median=None):
        """``PixelCube.create_threshold_mask(threshold, reference_pixel)`` of every cutout (reference targetpixelfile.py:680-742),
        equal to ``threshold_mask_from_median_image`` pixel for pixel, without leaving the device: the median images
        (``lk_cube_median_image_batch_dev`` over all cadences or those flagged in ``d_keep``), then the MAD cut, the 4-connected
        labelling and the choice of the region nearest to ``reference_pixel`` ((column, row), "center" or None) in
        ``lk_cube_threshold_mask_batch_dev``.  ``invert=True`` returns the complement ('background' is
        ``threshold_masks(0, None, invert=True)``).  ``to_host=True`` -> bool (B, ny, nx); ``to_host=False`` -> DeviceBuffers
        (mask B x npix bytes, count B int32, idx B x npix int32: the selected pixel numbers ascending, then -1), enqueued on the
        batch's stream.  Cutouts of more than ``_capi.CUBE_MASK_MAX_NPIX`` pixels take the host function (``to_host=True``
        only)."""
        from .correctors.pldcorrector import threshold_mask_from_median_image as from_median
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        if npix > _capi.CUBE_MASK_MAX_NPIX:
            if not to_host:
                raise ValueError("threshold_masks(to_host=False) holds the labels of at most %d pixels per cutout (got %d x %d)"
                                 % (_capi.CUBE_MASK_MAX_NPIX, ny, nx))
            med = self.median_images(d_keep)
            m = np.stack([from_median(im, threshold, reference_pixel) for im in med])
            return ~m if invert else m
        if isinstance(reference_pixel, str):
            if reference_pixel != "center":
                raise ValueError("reference_pixel must be (column, row), 'center' or None")
            reference_pixel = (nx / 2, ny / 2)
        d_med = _d_median if _d_median is not None else self._median_images_dev(d_keep)
        d_mask, d_cnt, d_idx = DeviceBuffer(h, B * npix), DeviceBuffer(h, B * 4), DeviceBuffer(h, B * npix * 4)
        use_ref = reference_pixel is not None
        _capi._check(_capi._lib.lk_cube_threshold_mask_batch_dev(
            h._h, B, ny, nx, _p(d_med), float(threshold), int(use_ref), float(reference_pixel[0]) if use_ref else 0.0,
            float(reference_pixel[1]) if use_ref else 0.0, int(bool(invert)), _p(d_mask), _p(d_cnt), _p(d_idx),
            _vp(self.stream or None)))
        if not to_host:
            return d_mask, d_cnt, d_idx         # (d_med goes back to the pool: its next user is ordered behind this stream's kernel)
        return self._get(d_mask, np.uint8, (B, ny, nx)).astype(bool)

    def _masks(self, spec, sap, d_keep, cache):
        """-> bool (ny, nx) shared by the batch, or bool (B, ny, nx): masks given per cutout, or a data-dependent spec evaluated
        on every cutout's own median image as ``PixelCube._parse_aperture_mask`` would — on the device (``threshold_masks``; the
        median images are computed once per call, kept in ``cache``, and never downloaded; B x npix mask bytes come back)."""
        m = self._shape_mask(spec, sap)
        if m is not None:
            return m
        if self.shape[2] * self.shape[3] <= _capi.CUBE_MASK_MAX_NPIX and "median" not in cache:
            cache["median"] = self._median_images_dev(d_keep)
        if spec == "background":
            return self.threshold_masks(0, None, d_keep, invert=True, _d_median=cache.get("median"))
        return self.threshold_masks(3, "center", d_keep, _d_median=cache.get("median"))

    def _stage_mask(self, spec, sap):
        """The mask ``spec`` (``_masks``) on the device -> (m, d_mask, mask_stride, staged): the bool (ny, nx) or (B, ny, nx) host
        mask, its bytes in HBM, the stride the C ABI takes (0: one mask shared by the batch) and the host array the upload reads.
        The upload is enqueued on the batch's stream and so is the kernel that reads it, so ``staged`` and ``d_mask`` both go to
        ``self._keep``.  ``_keep`` is emptied only where the batch has just synchronised its stream: ``synchronize()``,
        ``to_host()``, behind a C call that synchronises (``_aperture``) and at the end of a method whose last act on the stream
        is a download.  A method that returns another batch whose pending work reads the mask also hands both to that batch,
        which may outlive this one."""
        npix = self.shape[2] * self.shape[3]
        m = self._masks(spec, sap, None, {})
        d_mask, k = _upload(self.handle, m.reshape(-1, npix), self.stream, np.uint8)
        self._keep.extend([k, d_mask])
        return m, d_mask, npix if m.ndim == 3 else 0, k

    def _aperture(self, aperture_mask):
        """``lk_cube_aperture_batch_dev``: -> (d_flux32, d_err32, d_keep, kept[B], nonfinite[B])."""
        h, (B, N, ny, nx) = self.handle, self.shape
        _, d_mask, stride, _ = self._stage_mask(aperture_mask, True)
        d_f, d_e, d_k = DeviceBuffer(h, B * N * 4), DeviceBuffer(h, B * N * 4), DeviceBuffer(h, B * N)
        kept, dirty = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        _capi._check(_capi._lib.lk_cube_aperture_batch_dev(h._h, B, N, ny * nx, _p(self.d_flux), _p(self.d_flux_err), _p(d_mask),
                                                           stride, _p(d_f), _p(d_e), _p(d_k), _off_ptr(kept), _off_ptr(dirty),
                                                           _vp(self.stream or None)))           # (synchronises)
        self._keep = []
        n = int(kept[0])
        if np.any(kept != n):
            raise ValueError("pld_correct_batch needs cutouts with the same number of valid cadences")
        return d_f, d_e, d_k, n, dirty

    def _gather(self, d_f, d_e, d_k, n, pld_idx=None, P=0, bkg_idx=None, Pb=0, want_pld=False, want_bkg=False, knot_plan=None,
                ragged=False):
        """``lk_pld_gather_batch_dev`` -> dict of DeviceBuffers (time, y, err, lcf, pld, bkg, knots) + 'nonfinite'.  ``ragged``:
        ``pld_idx`` / ``bkg_idx`` are (DeviceBuffer, stride) pairs of -1-padded per-cutout lists and P / Pb the row pitch
        (``lk_pld_gather_ragged_batch_dev``)."""
        h, (B, N, ny, nx) = self.handle, self.shape
        out = dict(time=DeviceBuffer(h, B * n * 8), y=DeviceBuffer(h, B * n * 8), err=DeviceBuffer(h, B * n * 8),
                   lcf=DeviceBuffer(h, B * n * 4), pld=None, bkg=None, knots=None)
        if want_pld:
            out["pld"] = DeviceBuffer(h, B * n * P * 4)
        if want_bkg:
            out["bkg"] = DeviceBuffer(h, B * n * Pb * 4)
        lo = g = None
        n_inner = 0
        if knot_plan is not None:
            lo, g = knot_plan
            n_inner = len(lo)
            out["knots"] = DeviceBuffer(h, B * (n_inner + 2) * 8)

        def idx(a):
            return (None, 0) if a is None else (a.ctypes.data_as(_i32p), a.shape[1] if a.shape[0] > 1 else 0)

        def didx(a):
            return (None, 0) if a is None else (_p(a[0]), int(a[1]))

        (pi, ps), (bi, bs) = (didx(pld_idx), didx(bkg_idx)) if ragged else (idx(pld_idx), idx(bkg_idx))
        flag = np.zeros(1, dtype=np.int32)
        fn = _capi._lib.lk_pld_gather_ragged_batch_dev if ragged else _capi._lib.lk_pld_gather_batch_dev
        _capi._check(fn(
            h._h, B, N, ny * nx, n, _p(self.d_flux), _p(self.d_time), _p(d_f), _p(d_e), _p(d_k), int(P), pi,
            ps, int(Pb), bi, bs, n_inner, None if lo is None or not n_inner else lo.ctypes.data_as(_i32p),
            None if g is None or not n_inner else g.ctypes.data_as(_dp), _p(out["time"]), _p(out["y"]), _p(out["err"]),
            _p(out["lcf"]), _p(out["pld"]), _p(out["bkg"]), _p(out["knots"]), flag.ctypes.data_as(_i32p),
            _vp(self.stream or None)))      # (synchronises)
        out["nonfinite"] = bool(flag[0])
        return out

    # ---------------------------------------------------------------- aperture photometry
    def to_lightcurves(self, aperture_mask="all"):
        """``PixelCube.to_lightcurve(aperture_mask)`` of every cutout without its NaN cadences (what ``PLDCorrector.__init__``
        keeps, pldcorrector.py:109-120), resident -> ``DeviceLightCurveBatch`` (float64 = the float32 sums widened)."""
        from .device import DeviceLightCurveBatch
        B = len(self)
        d_f, d_e, d_k, n, _ = self._aperture(aperture_mask)
        if n < 1:
            raise ValueError("no cadence with a finite aperture flux")
        g = self._gather(d_f, d_e, d_k, n)
        return DeviceLightCurveBatch(g["time"], g["y"], g["err"], np.arange(B + 1, dtype=np.int64) * n,
                                     [dict(m) for m in self.meta], self.device, self.stream, nan_free=True,
                                     is_sorted=self.is_sorted)

    def estimate_centroids(self, aperture_mask="all", column=0, row=0, to_host=False, method="moments", return_peak=False):
        """``TargetPixelFile.estimate_centroids(aperture_mask, method)`` of every cadence of every cutout, ``column`` / ``row`` =
        the cutout's corner (``tpf.column`` / ``tpf.row``).  ``method="moments"`` (``lk_cube_centroids_batch_dev``): the flux-
        weighted mean pixel position inside the aperture; float64 sums, NaN pixels count as 0, a zero or NaN total gives NaN.
        ``method="quadratic"`` (``lk_cube_centroids_quadratic_batch_dev``): ``lightkurve.utils.centroid_quadratic``, the extremum
        of the quadratic through the 3 x 3 patch around the brightest pixel of ``flux * mask``; NaN for a NaN in the patch, a
        flat patch or a cadence without a value (nothing is raised); cutouts of at least 3 x 3 pixels.
        All N cadences, in the cube's order (``to_lightcurves`` drops NaN cadences: where it dropped any, select the same ones
        here).  -> (col, row): ``DeviceBuffer``s of B x N float64, what ``DeviceLightCurveBatch.sff_correct`` takes; or (B, N)
        numpy arrays with ``to_host=True``.  ``return_peak=True`` (quadratic only) adds a third item: B x N int32, the flat pixel
        index of the brightest pixel before the patch is clamped into the image, -1 for a cadence without a value."""
        if method not in ("moments", "quadratic"):
            raise ValueError("method must be 'moments' or 'quadratic' (got {!r})".format(method))
        if return_peak and method != "quadratic":
            raise ValueError("return_peak needs method='quadratic'")
        h, (B, N, ny, nx) = self.handle, self.shape
        _, d_mask, stride, _ = self._stage_mask(aperture_mask, True)
        d_c, d_r = DeviceBuffer(h, B * N * 8), DeviceBuffer(h, B * N * 8)
        d_p = DeviceBuffer(h, B * N * 4) if return_peak else None
        args = (h._h, B, N, ny * nx, nx, _p(self.d_flux), _p(d_mask), stride, float(column), float(row), _p(d_c), _p(d_r))
        if method == "quadratic":
            _capi._check(_capi._lib.lk_cube_centroids_quadratic_batch_dev(*args, _p(d_p), _vp(self.stream or None)))
        else:
            _capi._check(_capi._lib.lk_cube_centroids_batch_dev(*args, _vp(self.stream or None)))
        if not to_host:
            return (d_c, d_r, d_p) if return_peak else (d_c, d_r)
        out = (self._get(d_c, np.float64, (B, N)), self._get(d_r, np.float64, (B, N)))
        out = out + (self._get(d_p, np.int32, (B, N)),) if return_peak else out
        self._keep = []
        return out

    # ---------------------------------------------------------------- background
    def _background(self, aperture_mask, want_scatter, subtract):
        """One launch of ``lk_cube_background_batch_dev`` -> (masks bool (B, ny, nx), d_bkg, d_n_pixels, d_scatter or None,
        d_cube_out or None), enqueued on the batch's stream."""
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        m, d_mask, stride, _ = self._stage_mask(aperture_mask, False)
        d_bkg, d_n = DeviceBuffer(h, B * N * 4), DeviceBuffer(h, B * N * 4)
        d_sc = DeviceBuffer(h, B * N * 4) if want_scatter else None
        d_out = DeviceBuffer(h, B * N * npix * 4) if subtract else None
        _capi._check(_capi._lib.lk_cube_background_batch_dev(
            h._h, B, N, npix, _p(self.d_flux), _p(d_mask), stride, int(bool(want_scatter)), _p(d_bkg), _p(d_n), _p(d_sc), _p(d_out),
            _vp(self.stream or None)))
        return np.ascontiguousarray(np.broadcast_to(m, (B, ny, nx))), d_bkg, d_n, d_sc, d_out

    def estimate_background(self, aperture_mask="background", return_scatter=False, to_host=True):
        """``PixelCube.estimate_background(aperture_mask, return_scatter)`` of every cutout, value for value
        (``lk_cube_background_batch_dev``; ``TargetPixelFile.estimate_background``): per cadence the float32 ``np.nanmedian`` of the
        pixels in ``aperture_mask`` — 'background' (default: each cutout's own complement of ``threshold_masks(0, None)``, made on
        the device from the cube as it is), 'all', 'threshold', a bool (ny, nx) mask or one per cutout (B, ny, nx).  Returns a dict:
        ``flux`` float32 (B, N); ``n_pixels`` int32 (B, N), the masked pixels that are not NaN; ``mask`` bool (B, ny, nx);
        with ``return_scatter`` also ``scatter`` float32 (B, N), the median absolute deviation from ``flux``.  A cadence without a
        value is NaN.  ``to_host=False``: ``flux`` / ``n_pixels`` / ``scatter`` are ``DeviceBuffer``s enqueued on the batch's
        stream (``mask`` stays a host array: it is B x npix bytes and was made to be uploaded).  The cube does not move."""
        B, N = self.shape[:2]
        m, d_bkg, d_n, d_sc, _ = self._background(aperture_mask, return_scatter, False)
        out = {"flux": d_bkg, "n_pixels": d_n, "mask": m}
        if return_scatter:
            out["scatter"] = d_sc
        if to_host:
            for key, dt in (("flux", np.float32), ("n_pixels", np.int32), ("scatter", np.float32)):
                if key in out:
                    out[key] = self._get(out[key], dt, (B, N))
            self._keep = []
        return out

    def subtract_background(self, background=None, aperture_mask="background", return_background=False):
        """``PixelCube.subtract_background`` of every cutout -> a new ``DevicePixelCubeBatch`` whose ``d_flux`` is ``flux -
        bkg[:, :, None, None]`` in float32.  ``background=None``: the estimate over ``aperture_mask`` (see
        ``estimate_background``) and the subtraction in ONE launch — the cube is read once and written once.  Otherwise
        ``background`` is a host (B, N) array, a ``DeviceBuffer`` of B x N float32, or the dict ``estimate_background`` returned
        (either flavour), subtracted by ``lk_cube_subtract_rows_batch_dev``.  The result shares this batch's ``d_time`` and
        ``d_flux_err`` buffers (no method of the class writes them) and its host ``time``; ``meta`` is copied and gains, per
        cutout, ``BKG_SUBTRACTED`` = True, ``BKG_NPIX`` = the pixels of its mask (-1 when only values were given) and
        ``BKG_NAN_CADENCES``.  The B x N background values come to the host for that count (the call synchronises);
        ``return_background=True`` returns (batch, dict of ``flux`` (B, N) and, when a mask was used, ``n_pixels`` and ``mask``)."""
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        info = {}
        if background is None:
            m, d_bkg, d_n, _, d_out = self._background(aperture_mask, False, True)
            bkg = self._get(d_bkg, np.float32, (B, N))
            info = {"flux": bkg, "mask": m}
            if return_background:
                info["n_pixels"] = self._get(d_n, np.int32, (B, N))
            counts = m.reshape(B, npix).sum(axis=1)
        else:
            counts = np.full(B, -1)
            if isinstance(background, dict):
                if np.shape(background["mask"]) != (B, ny, nx):
                    raise ValueError("the background's masks have shape %r, this batch needs %r"
                                     % (np.shape(background["mask"]), (B, ny, nx)))
                counts = np.asarray(background["mask"], dtype=bool).reshape(B, npix).sum(axis=1)
                info = {key: background[key] for key in ("mask", "n_pixels") if key in background}
                background = background["flux"]
            keep = None
            if isinstance(background, DeviceBuffer):
                if background.nbytes != B * N * 4:
                    raise ValueError("a background of %d bytes for %d x %d float32 cadences" % (background.nbytes, B, N))
                d_rows = background
                bkg = self._get(d_rows, np.float32, (B, N))
            else:
                bkg = np.asarray(background, dtype=np.float32)
                if bkg.shape != (B, N):
                    raise ValueError("background must be (B, N) = %r, one value per cadence (got %r)" % ((B, N), bkg.shape))
                d_rows, keep = _upload(h, bkg, self.stream, np.float32)
            if isinstance(info.get("n_pixels"), DeviceBuffer):
                info["n_pixels"] = self._get(info["n_pixels"], np.int32, (B, N))
            info["flux"] = bkg
            d_out = DeviceBuffer(h, B * N * npix * 4)
            _capi._check(_capi._lib.lk_cube_subtract_rows_batch_dev(h._h, B, N, npix, _p(self.d_flux), _p(d_rows), _p(d_out),
                                                                    _vp(self.stream or None)))
        nan_cadences = np.isnan(bkg).sum(axis=1)
        meta = [dict(mb, BKG_SUBTRACTED=True, BKG_NPIX=int(counts[b]), BKG_NAN_CADENCES=int(nan_cadences[b]))
                for b, mb in enumerate(self.meta)]          # (the keys of PixelCube.subtract_background)
        out = DevicePixelCubeBatch(self.d_time, d_out, self.d_flux_err, self.time, self.shape, meta, self.device, self.stream,
                                   is_sorted=self.is_sorted)
        if background is not None:
            out._keep = [keep, d_rows]          # what the enqueued subtraction still reads
        return (out, info) if return_background else out

    # ---------------------------------------------------------------- difference images
    def _need_3x3(self):
        if self.shape[2] < 3 or self.shape[3] < 3:
            raise ValueError("the quadratic centroid needs cutouts of at least 3 x 3 pixels (got %d x %d)" % self.shape[2:])

    def _image_centroids(self, images, d_mask, stride, column, row, offsets_entry, lead):
        """The centroid of each of ``images`` = {key: (DeviceBuffer of B float64 images, method)}, method 1 quadratic, 0 moments,
        inside the staged mask, in the order of ``images``; then ``offsets_entry(handle, B, *lead, first pair, second pair, ...)``,
        the offset of the first image's centroid from the second's -> ({key: (d_col, d_row)}, d_offset, d_offset_pix, d_status),
        ``DeviceBuffer``s, enqueued."""
        h, (B, _, ny, nx), st = self.handle, self.shape, _vp(self.stream or None)
        cen = {}
        for key, (d_img, method) in images.items():
            cen[key] = (DeviceBuffer(h, B * 8), DeviceBuffer(h, B * 8))
            _capi._check(_capi._lib.lk_image_centroids_batch_dev(
                h._h, B, ny * nx, nx, _p(d_img), _p(d_mask), stride, float(column), float(row), method, _p(cen[key][0]),
                _p(cen[key][1]), _p(None), st))
        d_off, d_pix, d_status = DeviceBuffer(h, B * 16), DeviceBuffer(h, B * 8), DeviceBuffer(h, B * 4)
        first, second = list(cen.values())[:2]
        _capi._check(offsets_entry(h._h, B, *map(_p, tuple(lead) + first + second + (d_off, d_pix, d_status)), st))
        return cen, d_off, d_pix, d_status

    def _centroids_to_host(self, cen, d_off, d_pix):
        B = len(self)
        out = {key: np.stack([self._get(d, np.float64, (B,)) for d in pair], axis=1) for key, pair in cen.items()}
        out.update(offset=self._get(d_off, np.float64, (B, 2)), offset_pix=self._get(d_pix, np.float64, (B,)))
        return out

    def difference_images(self, period, transit_time, duration, in_width=0.5, out_inner=1.0, out_outer=2.0, aperture_mask="all",
                          column=0, row=0, to_host=True):
        """The transit difference image of every cutout and where it sits: is the dimming on the target's pixels or on a
        neighbour's?  ``period`` / ``transit_time`` / ``duration``: a scalar or one value per cutout (one box each).  Cadence i
        with time t has the phase x = (t - transit_time + period / 2) % period - period / 2 of ``create_transit_mask`` and is in
        transit where ``|x| < in_width * duration``, out of transit where ``out_inner * duration <= |x| < out_outer *
        duration``, neither elsewhere or for a NaN time (``0 < in_width <= out_inner < out_outer``, ``period != 0``).  Per pixel,
        float64 sums of the float32 values that are not NaN (``lk_cube_diffimage_batch_dev``): ``mean_in``, ``mean_out``,
        ``diff`` = mean_out - mean_in (positive where the dimming is) and ``diff_err`` = sqrt(sum_in e^2 / n_in^2 + sum_out e^2
        / n_out^2) from ``flux_err`` at the same values; a pixel without a value in a class is NaN where that class is needed.
        Then both centroid estimators of ``estimate_centroids`` on ``diff`` and ``mean_out`` inside ``aperture_mask``
        (``lk_image_centroids_batch_dev``).  Returns a dict: ``mean_in`` / ``mean_out`` / ``diff`` / ``diff_err`` (B, ny, nx);
        ``n_in`` / ``n_out`` (B,) int32, the cadences of each class; ``centroid_diff`` / ``centroid_out`` (B, 2) as (col, row),
        quadratic, and ``centroid_diff_moments`` / ``centroid_out_moments``; ``offset`` (B, 2) = centroid_diff - centroid_out and
        ``offset_pix`` (B,), its norm; ``status`` (B,) int32: 0 ok, 1 no in-transit cadence, 2 no out-of-transit cadence, 3 a
        quadratic centroid is undefined (nothing is raised for a cutout); ``cadence_class`` (B, N) uint8: 1 in, 2 out, 0 neither.
        ``to_host=False``: the images, ``offset``, ``offset_pix`` and ``cadence_class`` are ``DeviceBuffer``s and every centroid a
        pair (col, row) of ``DeviceBuffer``s of B float64, enqueued on the batch's stream; only the counts and the statuses come
        back.  A cutout's images have the same bits alone, in any batch and from run to run."""
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        if not (0 < in_width <= out_inner < out_outer):
            raise ValueError("need 0 < in_width <= out_inner < out_outer (got %r, %r, %r)" % (in_width, out_inner, out_outer))
        box = [_per_cutout(name, a, B) for name, a in (("period", period), ("transit_time", transit_time), ("duration", duration))]
        if np.any(box[0] == 0):
            raise ValueError("period must be non-zero")
        self._need_3x3()
        _, d_mask, stride, _ = self._stage_mask(aperture_mask, True)
        img = {key: DeviceBuffer(h, B * npix * 8) for key in ("mean_in", "mean_out", "diff", "diff_err")}
        d_cls, d_nin, d_nout = DeviceBuffer(h, B * N), DeviceBuffer(h, B * 4), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_cube_diffimage_batch_dev(
            h._h, B, N, npix, _p(self.d_time), _p(self.d_flux), _p(self.d_flux_err), box[0].ctypes.data_as(_dp),
            box[1].ctypes.data_as(_dp), box[2].ctypes.data_as(_dp), float(in_width), float(out_inner), float(out_outer),
            _p(d_cls), _p(img["mean_in"]), _p(img["mean_out"]), _p(img["diff"]), _p(img["diff_err"]), _p(d_nin), _p(d_nout),
            _vp(self.stream or None)))
        cen, d_off, d_pix, d_status = self._image_centroids(
            {"centroid_diff": (img["diff"], 1), "centroid_out": (img["mean_out"], 1), "centroid_diff_moments": (img["diff"], 0),
             "centroid_out_moments": (img["mean_out"], 0)}, d_mask, stride, column, row,
            _capi._lib.lk_diffimage_offsets_batch_dev, (d_nin, d_nout))
        out = {key: self._get(buf, np.int32, (B,)) for key, buf in (("n_in", d_nin), ("n_out", d_nout), ("status", d_status))}
        self._keep = []
        if not to_host:
            out.update(img, offset=d_off, offset_pix=d_pix, cadence_class=d_cls, **cen)
            return out
        for key, buf in img.items():
            out[key] = self._get(buf, np.float64, (B, ny, nx))
        out.update(self._centroids_to_host(cen, d_off, d_pix))
        out["cadence_class"] = self._get(d_cls, np.uint8, (B, N))
        return out

    # ---------------------------------------------------------------- amplitude images
    def amplitude_images(self, frequency, nterms=1, aperture_mask="all", column=0, row=0, to_host=True, freq_unit=None, peaks=None):
        """The amplitude image of every cutout and where it sits: is a periodic signal (a pulsation, a rotation signal, a
        contact binary) on the target's pixels or on a neighbour's?  The periodic twin of ``difference_images``; the numpy
        mirror is ``PixelCube.amplitude_image``.  ``frequency``: a scalar or one value per cutout in ``freq_unit`` (default
        1/d, the units of ``ls_model``); NaN or <= 0 skips the cutout (status 1).  With ``peaks`` (the float64[B, 2] array of
        ``to_periodogram_peaks(frequency, ...)`` of the cutouts' light curves) ``frequency`` is the grid that was searched and
        every cutout takes the frequency at its own maximum.  Per pixel (``lk_cube_ampimage_batch_dev``): an unweighted fit of
        [1, sin(2 pi m f (t - t_ref)), cos(2 pi m f (t - t_ref))], m = 1 .. ``nterms`` (1 .. 3), to the values that are not
        NaN at the cadences with a finite time; ``t_ref`` is each cutout's first finite time; float64 sums of the float32
        values, ``flux_err`` is not read.  Then both centroid estimators of ``estimate_centroids`` on ``amplitude[:, 0]`` and
        ``level`` inside ``aperture_mask`` (``lk_image_centroids_batch_dev``).  Returns a dict: ``theta`` (B, K, ny, nx), K = 2
        nterms + 1 (the bias, then sin 1, cos 1, ...); ``level`` (B, ny, nx) = y_mean + bias; ``amplitude`` / ``phase`` /
        ``amplitude_err`` / ``snr`` (B, nterms, ny, nx); ``chi2`` (B, ny, nx); ``n_used`` (B, ny, nx) int32; ``centroid_amp`` /
        ``centroid_level`` (B, 2) as (col, row), quadratic, and ``centroid_amp_moments`` / ``centroid_level_moments``;
        ``offset`` (B, 2) = centroid_amp - centroid_level and ``offset_pix`` (B,); ``frequency`` [1/d] and ``t_ref`` (B,);
        ``status`` (B,) int32: 0 ok, 1 skipped, 2 fewer than K + 1 cadences with a finite time, 3 a quadratic centroid is
        undefined (nothing is raised for a cutout or a pixel).  ``to_host=False``: the images, ``offset`` and ``offset_pix``
        are ``DeviceBuffer``s — ``theta`` laid out [K][B][npix] and the per-harmonic images [nterms][B][npix], every
        coefficient one block of B images — and every centroid a pair (col, row) of ``DeviceBuffer``s of B float64, enqueued
        on the batch's stream; only ``status`` comes back.  A cutout's images have the same bits alone, in any batch position
        and from run to run."""
        from .periodogram import _freq_unit_factor
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        if int(nterms) != nterms or not 1 <= int(nterms) <= 3:
            raise ValueError("nterms must be an integer 1 .. 3 (got %r)" % (nterms,))
        nterms = int(nterms)
        K = 2 * nterms + 1
        freq = np.asarray(frequency, dtype=np.float64)
        if peaks is not None:
            peaks = np.asarray(peaks, dtype=np.float64)
            if peaks.shape != (B, 2) or freq.ndim != 1 or freq.size < 2:
                raise ValueError("peaks must be the (%d, 2) array of to_periodogram_peaks(frequency) and frequency its grid" % B)
            at = np.where(np.isfinite(peaks[:, 1]), peaks[:, 1], -1).astype(np.int64)
            freq = np.where((at >= 0) & (at < freq.size), freq[np.clip(at, 0, freq.size - 1)], np.nan)
        f_day = _per_cutout("frequency", freq, B, finite=False) / _freq_unit_factor(freq_unit if freq_unit is not None else "1/d")
        self._need_3x3()
        t_ref = _first_finite_times(self.time)
        _, d_mask, stride, _ = self._stage_mask(aperture_mask, True)
        img = {key: DeviceBuffer(h, n * B * npix * 8) for key, n in (("theta", K), ("level", 1), ("amplitude", nterms), ("phase", nterms),
                                                                   ("amplitude_err", nterms), ("snr", nterms), ("chi2", 1))}
        d_used, d_fit = DeviceBuffer(h, B * npix * 4), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_cube_ampimage_batch_dev(
            h._h, B, N, npix, _p(self.d_time), _p(self.d_flux), f_day.ctypes.data_as(_dp), nterms, t_ref.ctypes.data_as(_dp),
            _p(img["theta"]), _p(img["level"]), _p(img["amplitude"]), _p(img["phase"]), _p(img["amplitude_err"]), _p(img["snr"]),
            _p(img["chi2"]), _p(d_used), _p(d_fit), _vp(self.stream or None)))
        cen, d_off, d_pix, d_status = self._image_centroids(      # (amplitude's first block is harmonic 1 of the batch)
            {"centroid_amp": (img["amplitude"], 1), "centroid_level": (img["level"], 1),
             "centroid_amp_moments": (img["amplitude"], 0), "centroid_level_moments": (img["level"], 0)},
            d_mask, stride, column, row, _capi._lib.lk_ampimage_offsets_batch_dev, (d_fit,))
        out = dict(status=self._get(d_status, np.int32, (B,)), frequency=f_day, t_ref=t_ref)
        self._keep = []
        if not to_host:
            out.update(img, n_used=d_used, offset=d_off, offset_pix=d_pix, **cen)
            return out
        for key, n in (("theta", K), ("amplitude", nterms), ("phase", nterms), ("amplitude_err", nterms), ("snr", nterms)):
            out[key] = np.ascontiguousarray(self._get(img[key], np.float64, (n, B, ny, nx)).transpose(1, 0, 2, 3))
        for key in ("level", "chi2"):
            out[key] = self._get(img[key], np.float64, (B, ny, nx))
        out["n_used"] = self._get(d_used, np.int32, (B, ny, nx))
        out.update(self._centroids_to_host(cen, d_off, d_pix))
        return out

    # ---------------------------------------------------------------- pixel periodograms
    def pixel_periodograms(self, frequency, normalization="amplitude", freq_unit=None, oversample_factor=None, return_power=True,
                           to_host=True, max_output_mb=4096):
        """One Lomb-Scargle spectrum per pixel of every cutout on ONE shared ``frequency`` grid, and where each peaks: which
        pixels vary, and at which frequency (what ``TargetPixelFile.plot_pixels(periodogram=True)`` loops for).  The numpy
        mirror and the definition is ``PixelCube.pixel_periodogram``: cadences with a non-finite time are dropped per cutout,
        pixel p is taken where its own flux is not NaN (``n_used[p]`` values, unit weights, ``flux_err`` is not read), its
        spectrum is the exact floating-mean GLS with lightkurve's ``normalization`` ('amplitude', ``frequency`` in 1/d by
        default; 'psd', microhertz by default, ``oversample_factor`` 1 by default).  Every grid value must be finite and > 0.
        The pixels of a cutout share the cadences, so four of the closed form's six sums are formed once per (cutout,
        frequency) and only two per pixel (``lk_cube_pixel_ls_batch_dev``); no transpose, no second copy of the cube.
        Returns a dict: ``power`` (B, F, ny, nx); ``peak_index`` (B, ny, nx) int32, the first index of the largest non-NaN
        power, -1 without one; ``peak_power`` and ``peak_frequency`` [1/d] (B, ny, nx), NaN there; ``n_used`` (B, ny, nx) int32;
        ``status`` (B,) int32: 0, or 2 for a cutout with fewer than 4 finite times (NaN spectra, ``n_used`` 0); ``t_ref`` (B,);
        ``frequency`` (F,) in 1/d.  ``return_power=False`` computes the peak images alone: nothing of the size of the power
        cube is written and the key is omitted; the peak images have the same bits either way.  ``ValueError`` when the power
        cube would exceed ``max_output_mb``.  ``to_host=False``: ``power`` ([B][F][npix]), ``peak_power``, ``peak_index`` and
        ``n_used`` are ``DeviceBuffer``s enqueued on the batch's stream, ``peak_frequency`` is omitted (``frequency[peak_index]``);
        only ``status`` comes back.  A cutout's outputs have the same bits alone, at any batch position and from run to run.
        No ``corrector_func`` runs per pixel (the reference's default removes outliers): clean the cube first, for instance
        with ``subtract_background``.  The hand-off to the fit at one frequency per cutout, for the pixel (row, col)::

            res = cubes.pixel_periodograms(grid)
            images = cubes.amplitude_images(res["peak_frequency"][:, row, col])"""
        from .periodogram import _freq_unit_factor
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        norms = {"amplitude": 2, "psd": 3}                          # LK_NORM_LK_AMPLITUDE, LK_NORM_LK_PSD
        if normalization not in norms:
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
        f_day = np.ascontiguousarray(freq / _freq_unit_factor(unit))
        F = int(f_day.size)
        if F * npix >= 2 ** 31:
            raise ValueError("a power cube of %d x %d values per cutout is too large" % (F, npix))
        power_bytes = B * F * npix * 8
        if return_power and power_bytes > max_output_mb * 2 ** 20:
            raise ValueError("the power cube of %d x %d x %d x %d float64 is %.0f MiB, more than max_output_mb = %r; raise it, pass "
                             "fewer cutouts or frequencies per call, or pass return_power=False for the peak images alone"
                             % (B, F, ny, nx, power_bytes / 2.0 ** 20, max_output_mb))
        t_ref = _first_finite_times(self.time)
        d_power = DeviceBuffer(h, power_bytes) if return_power else None
        d_peak, d_idx = DeviceBuffer(h, B * npix * 8), DeviceBuffer(h, B * npix * 4)
        d_used, d_status = DeviceBuffer(h, B * npix * 4), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_cube_pixel_ls_batch_dev(
            h._h, B, N, npix, _p(self.d_time), _p(self.d_flux), f_day.ctypes.data_as(_dp), F, norms[normalization], osf,
            t_ref.ctypes.data_as(_dp), _p(d_power), _p(d_peak), _p(d_idx), _p(d_used), _p(d_status), _vp(self.stream or None)))
        out = dict(status=self._get(d_status, np.int32, (B,)), t_ref=t_ref, frequency=f_day)
        if not to_host:
            out.update(peak_power=d_peak, peak_index=d_idx, n_used=d_used)
            if return_power:
                out["power"] = d_power
            return out
        if return_power:
            out["power"] = self._get(d_power, np.float64, (B, F, ny, nx))
        out["peak_power"] = self._get(d_peak, np.float64, (B, ny, nx))
        out["peak_index"] = self._get(d_idx, np.int32, (B, ny, nx))
        out["peak_frequency"] = np.where(out["peak_index"] >= 0, f_day[np.clip(out["peak_index"], 0, F - 1)], np.nan)
        out["n_used"] = self._get(d_used, np.int32, (B, ny, nx))
        return out

    # ---------------------------------------------------------------- PSF photometry
    def psf_photometry(self, star_col, star_row, sigma=None, shifts=None, aperture_mask="all", column=0, row=0, use_flux_err=True,
                       to_host=False, prf=None, prf_index=None):
        """Deblended PSF photometry per cadence of every cutout: the light curves of up to 8 blended stars at KNOWN positions,
        each without its neighbours, and a constant background — a weighted linear least-squares fit of pixel-integrated
        Gaussians to every cadence's image (``lk_cube_psf_photometry_batch_dev``; the numpy mirror and the definition is
        ``PixelCube.psf_photometry``).  The linear form of ``TargetPixelFile.to_lightcurve(method="prf")``: no position or
        width is fitted and no PRF file is read.  ``star_col`` / ``star_row``: [S] (the same stars in every cutout) or [B, S],
        S <= 8, in the coordinates of ``estimate_centroids`` with the same ``column`` / ``row`` (pixel (iy, ix) is centred on
        (column + ix, row + iy)); a star with a NaN coordinate is not part of its cutout, so cutouts with fewer stars are padded
        with NaN.  ``sigma``: a scalar, (sigma_col, sigma_row), or [B, 2], pixels.  ``shifts``: None, or a pair (shift_col,
        shift_row) of host arrays [B, N] or of ``DeviceBuffer``s of B x N float64, added to every star's position at that
        cadence.  ``estimate_centroids(to_host=False)`` returns that layout; offsets from centroids, on the host::

            c, r = cubes.estimate_centroids(to_host=True)
            shifts = (c - np.nanmedian(c, axis=1, keepdims=True), r - np.nanmedian(r, axis=1, keepdims=True))
            lcs, info = cubes.psf_photometry(star_col, star_row, 1.1, shifts=shifts)

        A cadence uses the pixels of ``aperture_mask`` whose flux is finite and, with ``use_flux_err``, whose flux_err is finite
        and > 0, weighted by 1 / flux_err^2 (else by 1).  Returns ``(lcs, info)``.  ``lcs``: a ``DeviceLightCurveBatch`` with
        one light curve per star, cutout-major (cutout b owns the rows ``star_off[b] : star_off[b + 1]``), N cadences each on
        its cutout's times, flux = the star's fitted flux and flux_err = sqrt((G^-1)_ss); a cadence that failed is NaN, so
        ``remove_nans()`` and the rest of the chain follow; ``meta`` is the cutout's plus ``STAR_INDEX``, ``STAR_COL``,
        ``STAR_ROW``.  ``info``: ``background`` and ``chi2`` (B x N float64), ``n_used`` (B x N int32, the used pixels),
        ``cadence_status`` (B x N int8: 0 ok, 1 the time or a shift is not finite, 2 n_used < S + 2, 3 singular), ``status`` (B
        int32: 1 when no cadence is ok) and ``star_off`` (B + 1 int32) — ``DeviceBuffer``s enqueued on the batch's stream, or
        host arrays with ``to_host=True``.  Nothing is raised per cadence.  A cutout's outputs have the same bits alone, at any
        batch position and from run to run.
        ``prf``: a ``TabulatedPRF`` in place of ``sigma`` (exactly one of the two, else ``ValueError``) — the model of every star
        is then interpolated from the table by Keys' cubic convolution (``lk_cube_prf_photometry_batch_dev``; the definition is
        ``TabulatedPRF``), which carries the wings and asymmetries of a mission PRF that no Gaussian width reproduces.  The
        table goes up once and stays on the ``TabulatedPRF``.  ``prf_index``: None (table 0), a scalar or [B], the table of every
        cutout.  Everything else, the return value included, is the same; ``psf_fit(prf=)`` fits the shifts with the same
        table, ``psf_width`` and ``psf_positions`` do not take one."""
        h, (B, N, ny, nx) = self.handle, self.shape
        pidx = _prf_index("psf_photometry", B, sigma, prf, prf_index)
        pos, part, sg, S_max = _psf_stars(B, star_col, star_row, sigma)
        keep = []
        d_shift = self._psf_shift_buffers(shifts, "shifts", keep)
        _, d_mask, stride, k = self._stage_mask(aperture_mask, False)
        keep += [k, d_mask]
        rows = int(part.sum())
        d_t, d_f, d_e = (DeviceBuffer(h, rows * N * 8) for _ in range(3))
        info = {key: DeviceBuffer(h, size) for key, _, size in _psf_info_spec(B, N, _PSF_INFO)}
        star_off = np.zeros(B + 1, dtype=np.int32)
        if prf is None:
            _capi._check(_capi._lib.lk_cube_psf_photometry_batch_dev(
                h._h, B, N, ny, nx, _p(self.d_time), _p(self.d_flux), _p(self.d_flux_err), _p(d_mask), stride, S_max,
                pos[0].ctypes.data_as(_dp), pos[1].ctypes.data_as(_dp), sg.ctypes.data_as(_dp), _p(d_shift[0]), _p(d_shift[1]),
                float(column), float(row), int(bool(use_flux_err)), star_off.ctypes.data_as(_i32p), _p(d_t), _p(d_f), _p(d_e),
                _p(info["background"]), _p(info["chi2"]), _p(info["n_used"]), _p(info["cadence_status"]), _p(info["status"]),
                _vp(self.stream or None)))
        else:
            n_prf, Ty, Tx = prf.samples.shape
            _capi._check(_capi._lib.lk_cube_prf_photometry_batch_dev(
                h._h, B, N, ny, nx, _p(self.d_time), _p(self.d_flux), _p(self.d_flux_err), _p(d_mask), stride, S_max,
                pos[0].ctypes.data_as(_dp), pos[1].ctypes.data_as(_dp), _p(_prf_device_table(prf, h, self.stream)), n_prf, Ty, Tx,
                prf.oversample, pidx.ctypes.data_as(_i32p), _p(d_shift[0]), _p(d_shift[1]), float(column), float(row),
                int(bool(use_flux_err)), star_off.ctypes.data_as(_i32p), _p(d_t), _p(d_f), _p(d_e), _p(info["background"]),
                _p(info["chi2"]), _p(info["n_used"]), _p(info["cadence_status"]), _p(info["status"]), _vp(self.stream or None)))
        return self._psf_results(pos, part, (d_t, d_f, d_e), keep + [d for d in d_shift if d is not None], info, _PSF_INFO,
                                 star_off, to_host)

    def psf_fit(self, star_col, star_row, sigma=None, shifts0=None, max_iter=10, tol=1e-7, max_step=0.5, max_shift=2.0,
                aperture_mask="all", column=0, row=0, use_flux_err=True, to_host=False, prf=None, prf_index=None):
        """PSF photometry that fits each cadence's pointing shift: ``psf_photometry`` with ONE common (column, row) shift of all
        stars per cadence fitted next to the fluxes and the background, by variable projection (``lk_cube_psf_fit_batch_dev``;
        the numpy mirror and the definition is ``PixelCube.psf_fit``).  The per-cadence motion shift of
        ``TargetPixelFile.to_lightcurve(method="prf")``: unlike the centroid of the whole blend (``estimate_centroids``) it is
        not biased by the blending and does not move when one star varies.  Per-star positions, the PSF width, rotation and
        a background gradient are not fitted.  Stars, ``sigma``, ``aperture_mask``, ``column`` / ``row`` and
        ``use_flux_err`` as in ``psf_photometry``.  ``shifts0``: None (start at 0) or a pair (shift_col, shift_row) of host
        arrays [B, N] or of ``DeviceBuffer``s of B x N float64, the initial shifts.  Up to ``max_iter`` (1 .. 64) Gauss-Newton
        steps per cadence, each component clamped to +-``max_step``; a cadence stops when its step is below ``tol`` (``tol`` =
        0: exactly ``max_iter`` steps), and fails when it moves more than ``max_shift`` from its start.  Returns ``(lcs,
        info)`` shaped like ``psf_photometry``'s, the fluxes, errors (conditional on the shift), ``background`` and ``chi2``
        being ``psf_photometry``'s at the fitted shifts.  ``info`` gains ``shift_col``, ``shift_row``, ``shift_col_err``,
        ``shift_row_err``, ``last_step`` (B x N float64) and ``n_iter`` (B x N int32); ``cadence_status``: 0 ok, 1 the time or
        an initial shift is not finite, 2 n_used < S + 4, 3 singular, 4 not converged, 5 left ``max_shift`` — a cadence that is
        not ok is NaN in every float output, the shifts included, while ``n_iter`` and ``last_step`` are reported for every
        cadence.  The shift buffers have the layout ``psf_photometry(shifts=)`` takes and feed ``sff_correct`` as a pointing
        history that no single star's variability biases::

            lcs, info = cubes.psf_fit(star_col, star_row, 1.1)
            again, _ = cubes.psf_photometry(star_col, star_row, 1.1, shifts=(info["shift_col"], info["shift_row"]))

        Nothing is raised per cadence.  A cutout's outputs have the same bits alone, at any batch position and from run to
        run.
        ``prf``: a ``TabulatedPRF`` in place of ``sigma`` (exactly one of the two, else ``ValueError``), ``prf_index`` as in
        ``psf_photometry``: the model and its derivative by the shift are interpolated from the table
        (``lk_cube_prf_fit_batch_dev``; the definition is ``PixelCube.psf_fit(prf=)``), so the fitted shifts carry no bias from
        a Gaussian stand-in and go straight into ``psf_photometry(prf=, shifts=)`` and ``sff_correct``::

            lcs, info = cubes.psf_fit(star_col, star_row, prf=prf)
            again, _ = cubes.psf_photometry(star_col, star_row, prf=prf, shifts=(info["shift_col"], info["shift_row"]))

        Everything else, the return value included, is the same."""
        from .correctors.pldcorrector import _psf_fit_parameters
        h, (B, N, ny, nx) = self.handle, self.shape
        pidx = _prf_index("psf_fit", B, sigma, prf, prf_index)
        pos, part, sg, S_max = _psf_stars(B, star_col, star_row, sigma)
        max_iter, tol, max_step, max_shift = _psf_fit_parameters(max_iter, tol, max_step, max_shift)
        keep = []
        d_shift = self._psf_shift_buffers(shifts0, "shifts0", keep)
        _, d_mask, stride, k = self._stage_mask(aperture_mask, False)
        keep += [k, d_mask]
        rows = int(part.sum())
        d_t, d_f, d_e = (DeviceBuffer(h, rows * N * 8) for _ in range(3))
        info = {key: DeviceBuffer(h, size) for key, _, size in _psf_info_spec(B, N, _PSF_FIT_INFO)}
        star_off = np.zeros(B + 1, dtype=np.int32)
        tail = (max_iter, tol, max_step, max_shift, float(column), float(row), int(bool(use_flux_err)), star_off.ctypes.data_as(_i32p),
                _p(d_t), _p(d_f), _p(d_e), _p(info["background"]), _p(info["chi2"]), _p(info["shift_col"]), _p(info["shift_row"]),
                _p(info["shift_col_err"]), _p(info["shift_row_err"]), _p(info["last_step"]), _p(info["n_iter"]), _p(info["n_used"]),
                _p(info["cadence_status"]), _p(info["status"]), _vp(self.stream or None))
        head = (h._h, B, N, ny, nx, _p(self.d_time), _p(self.d_flux), _p(self.d_flux_err), _p(d_mask), stride, S_max,
                pos[0].ctypes.data_as(_dp), pos[1].ctypes.data_as(_dp))
        if prf is None:
            _capi._check(_capi._lib.lk_cube_psf_fit_batch_dev(*(head + (sg.ctypes.data_as(_dp), _p(d_shift[0]), _p(d_shift[1])) + tail)))
        else:
            n_prf, Ty, Tx = prf.samples.shape
            _capi._check(_capi._lib.lk_cube_prf_fit_batch_dev(*(head + (
                _p(_prf_device_table(prf, h, self.stream)), n_prf, Ty, Tx, prf.oversample, pidx.ctypes.data_as(_i32p),
                _p(d_shift[0]), _p(d_shift[1])) + tail)))
        return self._psf_results(pos, part, (d_t, d_f, d_e), keep + [d for d in d_shift if d is not None], info, _PSF_FIT_INFO,
                                 star_off, to_host)

    def psf_width(self, star_col, star_row, sigma0, shifts=None, cadence_mask=None, max_iter=20, tol=1e-6, max_step=0.25,
                  min_sigma=0.2, max_sigma=5.0, aperture_mask="all", column=0, row=0, use_flux_err=True, to_host=True):
        """The PSF width of every cutout, fitted: ONE pair (sigma_col, sigma_row) per cutout, shared by all its cadences, by
        variable projection with every cadence's fluxes and background projected out (``lk_cube_psf_width_batch_dev``; the numpy
        mirror and the definition is ``PixelCube.psf_width``) — the ``sigma`` that ``psf_photometry`` and ``psf_fit`` take as
        given, the PSF scale of ``TargetPixelFile.to_lightcurve(method="prf")``.  The chain that calibrates itself::

            _, fit = cubes.psf_fit(star_col, star_row, sigma_guess)
            info = cubes.psf_width(star_col, star_row, sigma_guess, shifts=(fit["shift_col"], fit["shift_row"]))
            lcs, fit = cubes.psf_fit(star_col, star_row, info["sigma"])

        Stars, ``aperture_mask``, ``column`` / ``row`` and ``use_flux_err`` as in ``psf_photometry``.  ``sigma0``: a scalar,
        (sigma_col, sigma_row) or [B, 2], the start.  ``shifts``: None or a pair (shift_col, shift_row) of host arrays [B, N]
        or of ``DeviceBuffer``s of B x N float64 (what ``psf_fit`` returns; a cadence with a NaN shift is left out).
        ``cadence_mask``: None, a bool host array [B, N] or a ``DeviceBuffer`` of B x N bytes, the cadences to fit on — every
        tenth, say.  Up to ``max_iter`` (1 .. 64) Gauss-Newton steps per cutout, each component clamped to +-``max_step``; a
        cutout stops when its step is below ``tol`` (``tol`` = 0: exactly ``max_iter`` steps) and fails when a width leaves
        [``min_sigma``, ``max_sigma``].  Returns a dict: ``sigma`` and ``sigma_err`` (B, 2), ``sigma_cov``, ``chi2`` and
        ``last_step`` (B,) float64; ``trace`` (B, max_iter + 1, 2), the widths of every evaluation made, NaN beyond; ``n_iter``
        and ``n_cadences`` (B,) int32, ``n_pixels`` (B,) int64; ``cadence_status`` (B, N) int8: 0 contributed, 1 the time or a
        shift is not finite, 2 n_used < S + 2, 3 singular, 6 not selected; ``status`` (B,) int32: 0 ok, 1 no cadence
        contributed, 3 singular, 4 not converged, 5 left the bounds — a cutout that is not ok is NaN in ``sigma``,
        ``sigma_err``, ``sigma_cov`` and ``chi2``; nothing is raised per cutout.  Numpy arrays with ``to_host=True`` (16 bytes
        of widths per cutout), ``DeviceBuffer``s enqueued on the batch's stream with ``to_host=False``.  A cutout's outputs
        have the same bits alone, at any batch position and from run to run."""
        from .correctors.pldcorrector import _psf_width_parameters
        h, (B, N, ny, nx) = self.handle, self.shape
        pos, part, sg, S_max = _psf_stars(B, star_col, star_row, sigma0)
        max_iter, tol, max_step, min_sigma, max_sigma = _psf_width_parameters(max_iter, tol, max_step, min_sigma, max_sigma, sg)
        keep = []
        d_shift = self._psf_shift_buffers(shifts, "shifts", keep)
        d_cmask = self._psf_cadence_mask(cadence_mask, keep)
        _, d_mask, stride, _ = self._stage_mask(aperture_mask, False)           # kept in self._keep
        spec = _psf_width_spec(B, N, max_iter)
        out = {key: DeviceBuffer(h, int(np.prod(shape)) * np.dtype(dt).itemsize) for key, dt, shape in spec}
        _capi._check(_capi._lib.lk_cube_psf_width_batch_dev(
            h._h, B, N, ny, nx, _p(self.d_time), _p(self.d_flux), _p(self.d_flux_err), _p(d_mask), stride, S_max,
            pos[0].ctypes.data_as(_dp), pos[1].ctypes.data_as(_dp), sg.ctypes.data_as(_dp), _p(d_shift[0]), _p(d_shift[1]),
            _p(d_cmask), max_iter, tol, max_step, min_sigma, max_sigma, float(column), float(row), int(bool(use_flux_err)),
            _p(out["sigma"]), _p(out["sigma_err"]), _p(out["sigma_cov"]), _p(out["chi2"]), _p(out["last_step"]), _p(out["trace"]),
            _p(out["n_iter"]), _p(out["n_cadences"]), _p(out["n_pixels"]), _p(out["cadence_status"]), _p(out["status"]),
            _vp(self.stream or None)))
        keep += [d for d in d_shift if d is not None] + ([d_cmask] if d_cmask is not None else [])
        if not to_host:
            self._keep = self._keep + keep                              # what the enqueued fit still reads
            return out
        for key, dt, shape in spec:
            out[key] = self._get(out[key], dt, shape)
        self._keep = []
        return out

    def _psf_cadence_mask(self, cadence_mask, keep):
        """``cadence_mask`` of the PSF calls -> its bytes on the device or None: a bool host array [B, N], uploaded (what must
        outlive the upload is appended to ``keep``), or a ``DeviceBuffer`` of B x N bytes."""
        h, (B, N, _, _) = self.handle, self.shape
        if isinstance(cadence_mask, DeviceBuffer):
            if cadence_mask.nbytes != B * N:
                raise ValueError("a cadence_mask buffer of %d bytes for %d x %d cadences" % (cadence_mask.nbytes, B, N))
            return cadence_mask
        if cadence_mask is None:
            return None
        cm = np.asarray(cadence_mask)
        if cm.dtype != bool or cm.shape != (B, N):
            raise ValueError("cadence_mask must be a bool (B, N) = %r array (got %s %r)" % ((B, N), cm.dtype, cm.shape))
        d_cmask, k = _upload(h, cm.astype(np.uint8), self.stream, np.uint8)
        keep.append(k)
        return d_cmask

    def psf_positions(self, star_col, star_row, sigma, shifts=None, cadence_mask=None, fit_star=None, max_iter=20, tol=1e-6,
                      max_step=0.25, max_offset=1.0, aperture_mask="all", column=0, row=0, use_flux_err=True, to_host=True):
        """The positions of every cutout's stars, fitted: ONE (column, row) per fitted star, shared by all the cutout's cadences,
        by variable projection with every cadence's fluxes and background projected out (``lk_cube_psf_positions_batch_dev``;
        the numpy mirror and the definition is ``PixelCube.psf_positions``) — the ``star_col`` / ``star_row`` that
        ``psf_photometry``, ``psf_fit`` and ``psf_width`` take as given (a catalogue at another epoch, ``estimate_centroids`` of
        a blend, the peak images).  The chain that calibrates itself::

            _, fit = cubes.psf_fit(col, row, sigma_guess)
            shifts = (fit["shift_col"], fit["shift_row"])
            pos = cubes.psf_positions(col, row, sigma_guess, shifts=shifts)
            width = cubes.psf_width(pos["star_col"], pos["star_row"], sigma_guess, shifts=shifts)
            lcs, fit = cubes.psf_fit(pos["star_col"], pos["star_row"], width["sigma"])

        THE FIT IS CONDITIONAL ON THE SHIFTS (and on the width): a translation common to all stars is the same model as a
        constant added to every shift, the call never frees both, and ``fit_star`` can pin an anchor star.

        Stars (NaN = an empty slot), ``sigma`` (given, not fitted), ``aperture_mask``, ``column`` / ``row`` and ``use_flux_err``
        as in ``psf_photometry``; ``shifts`` and ``cadence_mask`` as in ``psf_width`` (host arrays or ``DeviceBuffer``s).
        ``fit_star``: None (every star present is fitted) or a bool array (S_max,) or (B, S_max); a star that is not fitted
        stays at its given position; a cutout with no fitted star is a ``ValueError``.  Up to ``max_iter`` (1 .. 64)
        Gauss-Newton steps per cutout, each component clamped to +-``max_step``; a cutout stops when its step is below ``tol``
        (``tol`` = 0: exactly ``max_iter`` steps) and fails when a position moves farther than ``max_offset`` from its start.
        Returns a dict, everything in the caller's slot layout: ``star_col`` / ``star_row`` (B, S_max): the fitted values, the
        given value bit for bit for a star that is not fitted, NaN in an empty slot; ``star_col_err`` / ``star_row_err`` (B,
        S_max) = sqrt((H^-1)_kk), NaN where the star is not fitted; ``position_cov`` (B, 2 S_max, 2 S_max) = H^-1 at index 2
        slot + axis; ``chi2`` and ``last_step`` (B,); ``trace`` (B, max_iter + 1, 2 S_max), the positions of every evaluation
        made, NaN beyond; ``n_iter`` and ``n_cadences`` (B,) int32, ``n_pixels`` (B,) int64; ``cadence_status`` (B, N) int8: 0
        contributed, 1 the time or a shift is not finite, 2 n_used < S + 2, 3 singular, 6 not selected; ``status`` (B,) int32: 0
        ok, 1 no cadence contributed, 3 singular, 4 not converged, 5 left ``max_offset`` — a cutout that is not ok is NaN in the
        fitted stars' positions, their errors, ``position_cov`` and ``chi2``; nothing is raised per cutout.  Numpy arrays with
        ``to_host=True``, ``DeviceBuffer``s enqueued on the batch's stream with ``to_host=False``.  A cutout's outputs have the
        same bits alone, at any batch position and from run to run."""
        from .correctors.pldcorrector import _psf_positions_parameters
        h, (B, N, ny, nx) = self.handle, self.shape
        pos, part, sg, S_max = _psf_stars(B, star_col, star_row, sigma)
        max_iter, tol, max_step, max_offset = _psf_positions_parameters(max_iter, tol, max_step, max_offset)
        if fit_star is None:
            fit = np.ones((B, S_max), dtype=bool)
        else:
            fit = np.asarray(fit_star)
            if fit.dtype != bool or fit.shape not in ((S_max,), (B, S_max)):
                raise ValueError("fit_star must be a bool array (S_max,) or (B, S_max) = %r (got %s %r)" % ((B, S_max), fit.dtype, fit.shape))
            fit = np.broadcast_to(fit, (B, S_max))
        if not np.all((fit & part).any(axis=1)):
            raise ValueError("cutouts %s have no fitted star" % np.flatnonzero(~(fit & part).any(axis=1)).tolist())
        fit8 = np.ascontiguousarray(fit, dtype=np.uint8)
        keep = []
        d_shift = self._psf_shift_buffers(shifts, "shifts", keep)
        d_cmask = self._psf_cadence_mask(cadence_mask, keep)
        _, d_mask, stride, _ = self._stage_mask(aperture_mask, False)           # kept in self._keep
        spec = _psf_positions_spec(B, N, S_max, max_iter)
        out = {key: DeviceBuffer(h, int(np.prod(shape)) * np.dtype(dt).itemsize) for key, dt, shape in spec}
        _capi._check(_capi._lib.lk_cube_psf_positions_batch_dev(
            h._h, B, N, ny, nx, _p(self.d_time), _p(self.d_flux), _p(self.d_flux_err), _p(d_mask), stride, S_max,
            pos[0].ctypes.data_as(_dp), pos[1].ctypes.data_as(_dp), sg.ctypes.data_as(_dp), _vp(fit8.ctypes.data), _p(d_shift[0]),
            _p(d_shift[1]), _p(d_cmask), max_iter, tol, max_step, max_offset, float(column), float(row), int(bool(use_flux_err)),
            _p(out["star_col"]), _p(out["star_row"]), _p(out["star_col_err"]), _p(out["star_row_err"]), _p(out["position_cov"]),
            _p(out["chi2"]), _p(out["last_step"]), _p(out["trace"]), _p(out["n_iter"]), _p(out["n_cadences"]), _p(out["n_pixels"]),
            _p(out["cadence_status"]), _p(out["status"]), _vp(self.stream or None)))
        keep += [d for d in d_shift if d is not None] + ([d_cmask] if d_cmask is not None else [])
        if not to_host:
            self._keep = self._keep + keep                              # what the enqueued fit still reads
            return out
        for key, dt, shape in spec:
            out[key] = self._get(out[key], dt, shape)
        self._keep = []
        return out

    def _psf_shift_buffers(self, shifts, name, keep):
        """``shifts`` / ``shifts0`` of the PSF calls -> [shift_col, shift_row] on the device (None, None without): a pair of
        host arrays [B, N], uploaded (what must outlive the upload is appended to ``keep``), or of ``DeviceBuffer``s."""
        h, (B, N) = self.handle, self.shape[:2]
        d_shift = [None, None]
        if shifts is not None:
            if len(shifts) != 2:
                raise ValueError("%s must be a pair (shift_col, shift_row)" % name)
            for i, a in enumerate(shifts):
                if isinstance(a, DeviceBuffer):
                    if a.nbytes != B * N * 8:
                        raise ValueError("a shift buffer of %d bytes for %d x %d float64 cadences" % (a.nbytes, B, N))
                    d_shift[i] = a
                else:
                    a = np.asarray(a, dtype=np.float64)
                    if a.shape != (B, N):
                        raise ValueError("%s must be (B, N) = %r arrays (got %r)" % (name, (B, N), a.shape))
                    d_shift[i], k = _upload(h, a, self.stream, np.float64)
                    keep.append(k)
        return d_shift

    def _psf_results(self, pos, part, curves, keep, info, spec, star_off, to_host):
        """The return value of the PSF calls: the light curves (one per star that took part, N cadences each) and ``info``
        (``DeviceBuffer``s, or host arrays with ``to_host``) with ``star_off``."""
        from .device import DeviceLightCurveBatch
        h, (B, N) = self.handle, self.shape[:2]
        rows = int(part.sum())
        meta = [dict(self.meta[b], STAR_INDEX=int(s), STAR_COL=float(pos[0][b, s]), STAR_ROW=float(pos[1][b, s]))
                for b in range(B) for s in np.flatnonzero(part[b])]
        lcs = DeviceLightCurveBatch(curves[0], curves[1], curves[2], np.arange(rows + 1, dtype=np.int64) * N, meta, self.device,
                                    self.stream, is_sorted=True if self.is_sorted else None)
        lcs._keep = list(keep)                                         # what the enqueued fit still reads
        if not to_host:
            info["star_off"], k = _upload(h, star_off, self.stream, np.int32)
            lcs._keep.append(k)
            return lcs, info
        for key, dt, _ in _psf_info_spec(B, N, spec):
            info[key] = self._get(info[key], dt, (B,) if key == "status" else (B, N))
        self._keep = []
        info["star_off"] = star_off
        return lcs, info

    # ---------------------------------------------------------------- PLD
    def pld_correct(self, aperture_mask="all", pld_aperture_mask="all", background_aperture_mask="all", pld_order=3,
                    pca_components=16, spline_n_knots=None, spline_degree=5, normalize_background_pixels=True,
                    restore_trend=True, cadence_mask=None, sigma=5, niters=5, to_host=True, ragged_masks=False):
        """``pld_correct_batch`` (same defaults and meaning; reference ``PLDCorrector(tpf, aperture_mask).correct(...)``,
        pldcorrector.py:304-427) on the resident cubes, bit-identical to it.  ``cadence_mask``: optional bool (B, n) over the
        KEPT cadences, True = used in the fit.  ``to_host=True`` -> (corrected[B, n], outlier_mask[B, n]) numpy arrays;
        ``to_host=False`` -> (``DeviceLightCurveBatch`` of the compacted times, the corrected flux and the SAP flux errors,
        ``DeviceBuffer`` of the B x n outlier bytes).  Each mask may also be a bool (B, ny, nx) array, one mask per cutout.
        ``ragged_masks=True`` accepts PLD / background masks that select DIFFERENT numbers of pixels per cutout — the usual case
        for 'threshold' / 'background' on real fields — through zero-padded pixel blocks and per-cutout counts
        (``lk_pld_gather_ragged_batch_dev``, ``lk_pld_correct_ragged_batch_dev``); every count must be at least
        ``pca_components`` (ValueError names the cutouts).  When all sizes are equal the call is the one without the keyword."""
        from .correctors.pldcorrector import _percentile_knot_plan, _ragged_index_lists
        from .device import DeviceLightCurveBatch
        if pca_components is None or pca_components < 1:
            raise NotImplementedError("pca_components must be >= 1 on the HIP path")
        if not self.is_sorted:
            raise ValueError("DevicePixelCubeBatch.pld_correct needs finite, non-decreasing times in every cutout (the spline "
                             "knots are gathered from sorted times); pld_correct_batch takes unsorted cutouts")
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        d_f, d_e, d_k, n, dirty = self._aperture(aperture_mask)
        if n < 2:
            raise ValueError("pld_correct needs at least two cadences with a finite aperture flux (got %d)" % n)
        cache = {}                                  # the median images over the KEPT cadences (the corrector sees tpf[~nan_mask])
        pm = self._masks(pld_aperture_mask, False, d_k, cache)
        bm = self._masks(background_aperture_mask, False, d_k, cache)
        counts_p, counts_b = pm.reshape(-1, npix).sum(axis=1), bm.reshape(-1, npix).sum(axis=1)
        ragged = len(set(counts_p.tolist())) > 1 or len(set(counts_b.tolist())) > 1
        if ragged and not ragged_masks:
            raise ValueError("pld_correct_batch: the per-cutout '%s' / '%s' masks select different numbers of pixels (%s PLD, %s "
                             "background); pass masks of one size or correct these cutouts one by one"
                             % (pld_aperture_mask, background_aperture_mask, sorted(set(counts_p.tolist())),
                                sorted(set(counts_b.tolist()))))
        P, Pb = int(counts_p.max()), int(counts_b.max())       # (ragged: the row pitch of the zero-padded blocks)
        same = pm.shape == bm.shape and np.array_equal(pm, bm)
        resident = n == N and not ragged            # full mask and no dropped cadence: the block IS the resident cube

        def index_lists(m, count):
            if count == npix or count == 0:
                return None
            return np.ascontiguousarray([np.flatnonzero(r) for r in m.reshape(-1, npix)], dtype=np.int32)

        keep = []
        d_pc = d_bc = None
        if ragged:
            # per-cutout ascending pixel lists padded with -1 to the pitch + the counts, uploaded once (B x (P + Pb + 2) int32)
            def lists(m, what):
                if not m.any():
                    return None, None
                idx, cnt = _ragged_index_lists(np.broadcast_to(m.reshape(-1, npix), (B, npix)), pca_components, what)
                d_i, k1 = _upload(h, idx, self.stream, np.int32)
                d_c, k2 = _upload(h, cnt, self.stream, np.int32)
                keep.extend([k1, k2])
                return (d_i, idx.shape[1]), d_c

            pld_idx, d_pc = lists(pm, "PLD")
            bkg_idx, d_bc = (pld_idx, d_pc) if same else lists(bm, "background")
        else:
            pld_idx, bkg_idx = index_lists(pm, P), index_lists(bm, Pb)
        want_pld = P > 0 and not (resident and P == npix)
        want_bkg = Pb > 0 and not same and not (resident and Pb == npix)
        if spline_n_knots is None:
            spline_n_knots = int(n / 50)
        plan = _percentile_knot_plan(n, int(spline_n_knots), int(spline_degree))
        g = self._gather(d_f, d_e, d_k, n, pld_idx, P, None if same else bkg_idx, 0 if same else Pb, want_pld, want_bkg, plan,
                         ragged=ragged)
        whole_image = (P == npix and not want_pld) or (Pb == npix and not want_bkg and not same)
        if g["nonfinite"] or (whole_image and dirty.any()):
            raise ValueError("pld_correct_batch needs finite pixels inside the masks")
        d_pld = g["pld"] if want_pld else (self.d_flux if P > 0 else None)
        d_bkg = d_pld if same else (g["bkg"] if want_bkg else self.d_flux)
        n_inner = len(plan[0])
        n_knots = n_inner + int(spline_degree) + 1
        K = _capi.pld_design_width(P, Pb, pld_order, pca_components, n_knots)
        d_cm = None
        if cadence_mask is not None:
            cm = np.ascontiguousarray(cadence_mask, dtype=np.uint8)
            if cm.shape != (B, n):
                raise ValueError("cadence_mask must be (B, n) = %s over the kept cadences (got %s)" % ((B, n), cm.shape))
            d_cm, k = _upload(h, cm, self.stream, np.uint8)
            keep.append(k)
        d_X = DeviceBuffer(h, B * n * K * 8)
        d_ps, d_mu, d_w = (DeviceBuffer(h, B * K * 8) for _ in range(3))
        d_model, d_corr = DeviceBuffer(h, B * n * 8), DeviceBuffer(h, B * n * 8)
        d_sp = DeviceBuffer(h, B * n * 8) if restore_trend else None
        d_outl = DeviceBuffer(h, B * n)
        args = (h._h, B, n, P, Pb, _p(d_pld), _p(d_bkg), _p(g["lcf"]), _p(g["time"]), _p(g["knots"]), n_inner, int(pld_order),
                int(pca_components), n_knots, int(spline_degree), int(bool(normalize_background_pixels)), K, _p(g["y"]), _p(g["err"]),
                _p(d_cm), float(sigma), int(niters), _p(d_X), _p(d_ps), _p(d_mu), _p(d_w), _p(d_model), _p(d_outl), _p(d_sp),
                _p(d_corr), _vp(self.stream or None))
        if ragged:
            _capi._check(_capi._lib.lk_pld_correct_ragged_batch_dev(*args, _p(d_pc), _p(d_bc)))
        else:
            _capi._check(_capi._lib.lk_pld_correct_batch_dev(*args))
        if to_host:
            return self._get(d_corr, np.float64, (B, n)), self._get(d_outl, np.uint8, (B, n)).astype(bool)
        out = DeviceLightCurveBatch(g["time"], d_corr, g["err"], np.arange(B + 1, dtype=np.int64) * n, [dict(m) for m in self.meta],
                                    self.device, self.stream, nan_free=True, is_sorted=True)
        # scratch and inputs the stream may still be reading: held until the batch is synchronised or dropped
        out._keep = keep + [d_X, d_ps, d_mu, d_w, d_model, d_sp, d_pld, d_bkg, g, d_f, d_e, d_k, pld_idx, bkg_idx, d_pc, d_bc, self]
        return out, d_outl


def _cube_times_sorted(time):
    """Finite, non-decreasing times in every cutout?  ``pld_correct`` takes the spline knots from SORTED times by index."""
    time = np.asarray(time, dtype=np.float64)
    return bool(np.all(np.isfinite(time)) and np.all(np.diff(time, axis=-1) >= 0))


def _check_cube_arrays(time, flux, flux_err):
    flux, flux_err = np.asarray(flux), np.asarray(flux_err)
    if flux.dtype != np.float32 or flux_err.dtype != np.float32:
        raise TypeError("DevicePixelCubeBatch holds float32 cubes (got %s / %s); pld_correct_batch takes the others"
                        % (flux.dtype, flux_err.dtype))
    time = np.ascontiguousarray(time, dtype=np.float64)
    if flux.ndim != 4 or flux.shape != flux_err.shape or time.shape != flux.shape[:2] or flux.shape[0] < 1:
        raise ValueError("time must be (B, N), flux and flux_err (B, N, ny, nx)")
    return time, np.ascontiguousarray(flux), np.ascontiguousarray(flux_err)
