"""Device-resident batch of light curves ("FITS -> ragged device arrays, remove_nans / normalize / bin /
fold / create_transit_mask on device").

``LightCurveBatch`` (ingest.py) keeps the packed arrays on the HOST: every stage of a chained pipeline is H2D -> kernel ->
D2H.  ``DeviceLightCurveBatch`` uploads once and chains the ``lk_*_batch_dev`` entry points on ONE stream of ONE handle;
only what the caller asks back crosses PCIe.  The reference loop this replaces (per object, per stage, on the host):

    for lc in collection:                                     # src/lightkurve/collections.py:145
        lc = lc.remove_nans().normalize()                     # lightcurve.py:1300-1327, 1216-1292
        lc = lc.flatten(window_length=401)                    # :943-1078
        pg = lc.to_periodogram(frequency=f)                   # :2490-2535 -> periodogram.py:636-989
        lc.fold(period=pg.period_at_max_power)                # :1089-1214

    batch = DeviceLightCurveBatch.from_lightcurves(lcs)       # or .from_fits(paths) / .from_batch(host_batch)
    flat = batch.remove_nans().normalize().flatten(window_length=401)
    peaks = flat.to_periodogram_peaks(f)                      # float64[B, 2] on the host: 16 B per target cross PCIe
    folded = flat.fold(period=1 / f[peaks[:, 1].astype(int)]).to_host()

No torch: device memory, copies and the stream come from liblkhip.so itself (``lk_dev_alloc`` / ``lk_memcpy_*`` /
``lk_stream_*``).  Results are bit-identical to the staged host path — the same kernels run on the same numbers.
"""
import ctypes
import math

import numpy as np

from . import _capi
from . import fillgaps as _fg
from . import foldbin as _fb
from . import packed
from . import periodogram as _pg
from . import river as _rv
from . import seismology as _seis
from .cotrend import CotrendMixin, _alpha_per_target, _cadenceno_array, _cbv_columns  # noqa: F401  (names others import from here)
from .devmem import DeviceBuffer, _Pool, _ip, _off_ptr, _pool, _upload, _vp, release_device_pool  # noqa: F401

__all__ = ["DeviceBuffer", "DeviceLightCurveBatch", "DeviceFoldedBatch", "DevicePhaseCurveBatch", "DeviceBLSResult",
           "DevicePeriodogramBatch", "DevicePixelCubeBatch", "release_device_pool"]

_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)


# ------------------------------------------------------------------------------------------------ the batch
class DeviceLightCurveBatch(CotrendMixin):
    """B light curves as packed float64 arrays IN HBM (``d_time`` / ``d_flux`` / ``d_flux_err``: ``DeviceBuffer``) plus the
    prefix offsets ``n_off`` on the host (every launcher sizes its grid from them).  All work goes to ``stream`` (an opaque
    stream handle: ``0`` = the null stream, ``lk_stream_create``'s, or e.g. ``torch.cuda.current_stream().cuda_stream``) of
    the process's handle for ``device``."""

    def __init__(self, d_time, d_flux, d_flux_err, n_off, meta=None, device=0, stream=0, nan_free=False, is_sorted=None):
        self.handle = _capi.Handle.get(device)
        self.device = int(device)
        self.stream = int(stream or 0)
        self.d_time, self.d_flux, self.d_flux_err = d_time, d_flux, d_flux_err
        self.n_off = np.ascontiguousarray(n_off, dtype=np.int64)
        if self.n_off.ndim != 1 or self.n_off.size < 1 or self.n_off[0] != 0 or np.any(np.diff(self.n_off) < 0):
            raise ValueError("n_off must be non-decreasing prefix offsets starting at 0")
        need = int(self.n_off[-1]) * 8
        for b in (d_time, d_flux, d_flux_err):
            if b is not None and b.capacity < need:
                raise ValueError("device buffer smaller than the batch it is said to hold")
        self.meta = list(meta) if meta is not None else [{} for _ in range(len(self))]
        self.nan_free = bool(nan_free)          # no NaN flux: the periodogram front ends need not compact first
        self.is_sorted = is_sorted              # times non-decreasing per light curve (None: not checked yet)
        self.d_quality = None                   # int32 flags (from_fits), carried through remove_nans / normalize
        self.d_cadenceno = None                 # int32 cadence numbers (from_fits / from_arrays(cadenceno=)), carried likewise
        self.median_flux = None                 # DeviceBuffer float64[B] after remove_nans / normalize
        self._keep = []                         # host staging the stream may still be reading

    # ---------------------------------------------------------------- construction
    @classmethod
    def from_arrays(cls, time, flux, flux_err, n_off, meta=None, device=0, stream=0, cadenceno=None):
        """H2D once: packed host arrays (page-locked ones from ``_capi.pinned_empty`` / the staging pool go by DMA).
        ``cadenceno``: integer cadence numbers, one per cadence (what ``cbv_correct(cadenceno=)`` aligns by)."""
        time = np.ascontiguousarray(time, dtype=np.float64)
        n_off = _capi._offsets(n_off, time.size)
        h = _capi.Handle.get(device)
        srt = packed.check_sorted(time, n_off)
        bufs, keep = [], []
        for a in (time, flux, flux_err):
            if a is None:
                bufs.append(None)
                continue
            if np.shape(a) != time.shape:
                raise ValueError("time, flux, flux_err must be 1-D arrays of one length")
            b, k = _upload(h, a, stream)
            bufs.append(b), keep.append(k)
        if cadenceno is not None:
            cad = _cadenceno_array(cadenceno, time.size, "cadenceno")
        out = cls(bufs[0], bufs[1], bufs[2], n_off, meta, device, stream, is_sorted=srt)
        if cadenceno is not None:
            out.d_cadenceno, k = _upload(h, cad, stream, np.int32)
            keep.append(k)
        out._keep = keep
        return out

    @classmethod
    def from_lightcurves(cls, lcs, device=0, stream=0):
        """From an iterable of light curves (this package's or lightkurve's own): one concatenation per column into the
        page-locked staging pool, then ONE upload."""
        lcs = list(lcs)
        meta = [dict(getattr(lc, "meta", {}) or {}) for lc in lcs]
        (t, f, e), off = packed.pack_columns(lcs, ("time", "flux", "flux_err"), pinned="auto", pool_prefix="devbatch")
        out = cls.from_arrays(t, f, e, off, meta, device, stream)
        out.synchronize()        # the staging pool is reused by the next packing call
        out._keep = []
        return out

    @classmethod
    def from_batch(cls, batch, device=0, stream=0):
        """From a host ``LightCurveBatch``."""
        out = cls.from_arrays(batch.time, batch.flux, batch.flux_err, batch.n_off, [dict(m) for m in batch.meta], device, stream,
                              cadenceno=getattr(batch, "cadenceno", None))
        if getattr(batch, "quality", None) is not None:
            out.d_quality, k = _upload(out.handle, batch.quality, stream, np.int32)
            out._keep.append(k)
        return out

    @classmethod
    def from_fits(cls, paths, flux_column=None, quality_bitmask="default", ext=1, device=0, stream=0):
        """Light-curve FITS files -> a device-resident batch (``LightCurveBatch.from_fits`` without the way back: reference
        ``lk.read(path)`` per file, src/lightkurve/io/generic.py:21-207, io/kepler.py, io/tess.py).  The host parses the
        headers; the tables' bytes go to HBM as they are and ``lk_fits_unpack_batch_dev`` turns them into the arrays.  When
        every table has a CADENCENO column the kept cadences' numbers become ``d_cadenceno`` (``lk_fits_cadenceno_batch_dev``)."""
        from . import fitsio
        h = _capi.Handle.get(device)
        raws, descs, masks, meta, cadcols = [], [], [], [], []
        for path in paths:
            tab = fitsio.read_fits_table(path, ext=ext)
            desc, bitmask, mission = fitsio.lightcurve_columns(tab, flux_column=flux_column, quality_bitmask=quality_bitmask)
            raws.append(tab.raw), descs.append(desc), masks.append(bitmask), cadcols.append(fitsio.int_column(tab, "cadenceno"))
            meta.append({"FILENAME": str(path), "LABEL": tab.primary.get("OBJECT"),
                         "MISSION": tab.primary.get("MISSION", tab.primary.get("TELESCOP")), "RA": tab.primary.get("RA_OBJ"),
                         "DEC": tab.primary.get("DEC_OBJ"), "QUALITY_BITMASK": quality_bitmask,
                         "BJDREFI": tab.header.get("BJDREFI"), "READER_MISSION": mission})
        B = len(raws)
        desc = np.ascontiguousarray(descs, dtype=np.int32).reshape(B, 10)
        mask = np.ascontiguousarray(masks, dtype=np.int64).reshape(B)
        raw_off = np.zeros(B + 1, dtype=np.int64)
        for b, r in enumerate(raws):
            nbytes = int(desc[b, 0]) * int(desc[b, 1])
            if np.asarray(r).size != nbytes:
                raise ValueError("file %d: %d bytes of table data, descriptor says %d rows x %d bytes"
                                 % (b, np.asarray(r).size, desc[b, 1], desc[b, 0]))
            raw_off[b + 1] = raw_off[b] + ((nbytes + 3 + 15) // 16) * 16
        try:
            raw = _capi.pinned_pool("devbatch:fits", int(raw_off[-1]), np.uint8)
        except (OSError, RuntimeError, MemoryError):
            raw = np.empty(int(raw_off[-1]), dtype=np.uint8)
        for b, r in enumerate(raws):
            r = np.asarray(r, dtype=np.uint8).reshape(-1)
            raw[raw_off[b]:raw_off[b] + r.size] = r
            raw[raw_off[b] + r.size:raw_off[b + 1]] = 0
        rows = int(desc[:, 1].sum())
        d_raw = DeviceBuffer(h, raw.nbytes)
        d_raw.upload(raw, stream)
        d_t, d_f, d_e = (DeviceBuffer(h, rows * 8) for _ in range(3))
        d_q = DeviceBuffer(h, rows * 4)
        new_off = np.zeros(B + 1, dtype=np.int64)
        _capi._check(_capi._lib.lk_fits_unpack_batch_dev(h._h, B, _vp(d_raw.ptr), _off_ptr(raw_off), desc.ctypes.data_as(_i32p),
                                                         _off_ptr(mask), _vp(d_t.ptr), _vp(d_f.ptr), _vp(d_e.ptr), _vp(d_q.ptr),
                                                         _off_ptr(new_off), _vp(stream or None)))     # (synchronises)
        out = cls(d_t, d_f, d_e, new_off, meta, device, stream)
        out.d_quality = d_q
        if B and all(c is not None for c in cadcols):      # every table has CADENCENO: decoded from the same bytes
            col = np.ascontiguousarray(cadcols, dtype=np.int32).reshape(B, 2)
            d_c = DeviceBuffer(h, max(int(new_off[-1]), 1) * 4)
            _capi._check(_capi._lib.lk_fits_cadenceno_batch_dev(h._h, B, _vp(d_raw.ptr), _off_ptr(raw_off), desc.ctypes.data_as(_i32p),
                                                                col.ctypes.data_as(_i32p), _off_ptr(mask), _off_ptr(new_off),
                                                                _vp(d_c.ptr), _vp(stream or None)))
            out.d_cadenceno = d_c
            out._keep = [d_raw]          # the decode may still be reading the tables' bytes
        return out

    # ---------------------------------------------------------------- plumbing
    def __len__(self):
        return len(self.n_off) - 1

    @property
    def n_cadences(self):
        return int(self.n_off[-1])

    def synchronize(self):
        _capi._check(_capi._lib.lk_stream_synchronize(self.handle._h, _vp(self.stream or None)))
        self._keep = []

    def _new(self, d_time, d_flux, d_err, n_off, **kw):
        out = DeviceLightCurveBatch(d_time, d_flux, d_err, n_off, [dict(m) for m in self.meta], self.device, self.stream, **kw)
        return out

    def _host(self, buf, dtype=np.float64):
        if buf is None:
            return None
        return buf.download(dtype, self.n_cadences, stream=self.stream)

    def time_host(self):
        return self._host(self.d_time)

    def flux_host(self):
        return self._host(self.d_flux)

    def flux_err_host(self):
        return self._host(self.d_flux_err)

    def quality_host(self):
        return self._host(self.d_quality, np.int32)

    def cadenceno_host(self):
        """The cadence numbers of all cadences of the batch (int32), or None when the batch carries none."""
        return self._host(self.d_cadenceno, np.int32)

    def _carry(self, out):
        """The per-cadence integer columns onto a batch with the same cadences."""
        out.d_quality, out.d_cadenceno = self.d_quality, self.d_cadenceno
        return out

    def to_host(self):
        """D2H of the three columns -> ``LightCurveBatch`` (what a caller asks back at the END of a chain)."""
        from .ingest import LightCurveBatch
        n = self.n_cadences
        e = self.flux_err_host() if self.d_flux_err is not None else np.full(n, np.nan)
        out = LightCurveBatch(self.time_host(), self.flux_host(), e, self.n_off.copy(), [dict(m) for m in self.meta])
        if self.d_quality is not None:
            out.quality = self.quality_host()
        if self.d_cadenceno is not None:
            out.cadenceno = self.cadenceno_host()
        return out

    def _sorted(self):
        if self.is_sorted is None:
            B = len(self)
            desc = np.zeros(max(B, 1), dtype=np.int64)
            _capi._check(_capi._lib.lk_segment_probe_batch_dev(self.handle._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), None,
                                                               _off_ptr(desc), None, _vp(self.stream or None)))
            self.is_sorted = not bool(desc[:B].any())
        return self.is_sorted

    # ---------------------------------------------------------------- remove_nans / normalize
    def _ingest(self, normalize):
        h, B, n = self.handle, len(self), self.n_cadences
        d_t, d_f = DeviceBuffer(h, n * 8), DeviceBuffer(h, n * 8)
        d_e = DeviceBuffer(h, n * 8) if self.d_flux_err is not None else None
        d_med = DeviceBuffer(h, max(B, 1) * 8)
        new_off = np.zeros(B + 1, dtype=np.int64)
        _capi._check(_capi._lib.lk_ingest_batch_dev(
            h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), _vp(self.d_flux.ptr),
            _vp(self.d_flux_err.ptr if self.d_flux_err is not None else None), int(bool(normalize)), _vp(d_t.ptr), _vp(d_f.ptr),
            _vp(d_e.ptr if d_e is not None else None), _off_ptr(new_off), _vp(d_med.ptr), _vp(self.stream or None)))
        out = self._new(d_t, d_f, d_e, new_off, nan_free=True, is_sorted=self.is_sorted)
        out.median_flux = d_med
        for name in ("d_quality", "d_cadenceno"):
            src = getattr(self, name)
            if src is not None:
                d_q = DeviceBuffer(h, n * 4)
                cin, cout = (_vp * 1)(src.ptr), (_vp * 1)(d_q.ptr)
                _capi._check(_capi._lib.lk_compact_columns_batch_dev(h._h, B, _off_ptr(self.n_off), _off_ptr(new_off),
                                                                     _vp(self.d_flux.ptr), 1, 4, cin, cout, _vp(self.stream or None)))
                setattr(out, name, d_q)
        return out

    def remove_nans(self):
        """Every light curve without the cadences whose flux is NaN (reference lightcurve.py:1300-1327); repacked in HBM."""
        return self._ingest(False)

    def normalize(self):
        """flux and flux_err divided by nanmedian(flux) per light curve (reference :1216-1292); NaN-flux cadences are
        dropped first, as ``LightCurveBatch.normalize`` does."""
        out = self._ingest(True)
        for m in out.meta:
            m["NORMALIZED"] = True
        return out

    # ---------------------------------------------------------------- flatten
    def flatten_trend(self, window_length=101, polyorder=2, break_tolerance=5, niters=3, sigma=3, mask=None):
        """The trend ``LightCurve.flatten`` divides by (reference :996-1063) -> ``DeviceBuffer`` float64[sum N].
        ``mask``: bool / uint8 array over all cadences of the batch (host, uploaded) or a ``DeviceBuffer`` of bytes,
        1 = excluded from the fit."""
        if polyorder >= window_length:
            polyorder = window_length - 1
        if window_length % 2 != 1:
            raise ValueError("window_length must be odd (scipy.signal.savgol_filter with mode='interp')")
        if not self._sorted():
            raise ValueError("flatten needs the light curve sorted by time")
        h, n = self.handle, self.n_cadences
        d_m = None
        if mask is not None:
            if isinstance(mask, DeviceBuffer):
                d_m = mask
            else:
                mk = np.ascontiguousarray(mask, dtype=np.uint8)
                if mk.shape != (n,):
                    raise ValueError("mask must have one entry per cadence (got shape %s, need (%d,))" % (mk.shape, n))
                d_m, k = _upload(h, mk, self.stream, np.uint8)
                self._keep.append(k)
        bt = float("nan") if break_tolerance is None else float(break_tolerance)
        d_tr = DeviceBuffer(h, n * 8)
        _capi._check(_capi._lib.lk_savgol_trend_batch_dev(h._h, len(self), _off_ptr(self.n_off), _vp(self.d_time.ptr),
                                                          _vp(self.d_flux.ptr), _vp(d_m.ptr if d_m is not None else None),
                                                          int(window_length), int(polyorder), bt, int(niters), float(sigma),
                                                          _vp(d_tr.ptr), None, _vp(self.stream or None)))
        return d_tr

    def flatten(self, window_length=101, polyorder=2, return_trend=False, break_tolerance=5, niters=3, sigma=3, mask=None):
        """``lc.flatten(...)`` for the whole batch, result resident: flux / trend and flux_err / trend (reference
        :1064-1070).  ``return_trend``: also a batch whose flux is the trend (the reference's ``trend_lc``)."""
        d_tr = self.flatten_trend(window_length, polyorder, break_tolerance, niters, sigma, mask)
        h, n = self.handle, self.n_cadences
        d_f = DeviceBuffer(h, n * 8)
        d_e = DeviceBuffer(h, n * 8) if self.d_flux_err is not None else None
        _capi._check(_capi._lib.lk_flatten_apply_batch_dev(h._h, n, _vp(self.d_flux.ptr),
                                                           _vp(self.d_flux_err.ptr if self.d_flux_err is not None else None),
                                                           _vp(d_tr.ptr), _vp(d_f.ptr), _vp(d_e.ptr if d_e is not None else None),
                                                           _vp(self.stream or None)))
        out = self._carry(self._new(self.d_time, d_f, d_e, self.n_off, nan_free=False, is_sorted=self.is_sorted))
        for m in out.meta:
            m["NORMALIZED"] = True
        if return_trend:
            tr = self._new(self.d_time, d_tr, self.d_flux_err, self.n_off, nan_free=False, is_sorted=self.is_sorted)
            return out, tr
        return out

    # ---------------------------------------------------------------- outliers / select / CDPP
    def outlier_mask(self, sigma=5.0, sigma_lower=None, sigma_upper=None, maxiters=5, to_host=False):
        """``astropy.stats.sigma_clip(flux, sigma, sigma_lower, sigma_upper, maxiters).mask`` per light curve (what
        ``LightCurve.remove_outliers`` removes, reference :1430-1556): 1 = clipped or not finite -> ``DeviceBuffer`` of bytes
        over this batch's cadences (usable as ``select(mask, invert=True)`` / ``flatten(mask=...)``), or a host bool array
        with ``to_host=True``.  ``None`` bounds fall back to ``sigma``; ``maxiters=None``: until a round removes nothing."""
        lo, hi, mi = _capi.clip_bounds(sigma, sigma_lower, sigma_upper, maxiters)
        h, n = self.handle, self.n_cadences
        d_m = DeviceBuffer(h, max(n, 1))
        _capi._check(_capi._lib.lk_outlier_mask_batch_dev(h._h, len(self), _off_ptr(self.n_off), _vp(self.d_flux.ptr), lo, hi, mi,
                                                          _vp(d_m.ptr), _vp(self.stream or None)))
        if not to_host:
            return d_m
        return d_m.download(np.uint8, n, stream=self.stream).astype(bool)

    def select(self, mask, invert=False):
        """``lc[mask]`` (``invert``: ``lc[~mask]``) for every light curve, resident: ``mask`` is a host bool / uint8 array over
        the ``n_cadences`` of this batch or a ``DeviceBuffer`` of that many bytes (``outlier_mask`` /
        ``DeviceBLSResult.transit_mask(to_host=False)`` / ``create_transit_mask(to_host=False)``).  time, flux, flux_err and
        the quality flags are repacked in HBM, order kept (``lk_select_columns_batch_dev``; the call synchronises: the new
        offsets come back).  ``median_flux`` does not carry over."""
        h, B, n = self.handle, len(self), self.n_cadences
        if isinstance(mask, DeviceBuffer):
            if mask.nbytes != max(n, 1):
                raise ValueError("mask holds %d bytes, the batch has %d cadences" % (mask.nbytes, n))
            d_m = mask
        else:
            mk = np.asarray(mask)
            if mk.dtype != np.bool_ and mk.dtype != np.uint8:
                raise ValueError("mask must be a bool or uint8 array (got %s)" % mk.dtype)
            if mk.shape != (n,):
                raise ValueError("mask must have one entry per cadence (got shape %s, need (%d,))" % (mk.shape, n))
            d_m, _k = _upload(h, mk, self.stream, np.uint8)
        cols = [(self.d_time, 8), (self.d_flux, 8)]
        if self.d_flux_err is not None:
            cols.append((self.d_flux_err, 8))
        if self.d_quality is not None:
            cols.append((self.d_quality, 4))
        if self.d_cadenceno is not None:
            cols.append((self.d_cadenceno, 4))
        outs = [DeviceBuffer(h, max(n, 1) * eb) for _c, eb in cols]
        cin = (_vp * len(cols))(*[c.ptr for c, _eb in cols])
        cout = (_vp * len(cols))(*[c.ptr for c in outs])
        elem = np.ascontiguousarray([eb for _c, eb in cols], dtype=np.int32)
        new_off = np.zeros(B + 1, dtype=np.int64)
        _capi._check(_capi._lib.lk_select_columns_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(d_m.ptr), int(bool(invert)), len(cols),
                                                            elem.ctypes.data_as(_i32p), cin, cout, _off_ptr(new_off),
                                                            _vp(self.stream or None)))      # (synchronises)
        it = iter(outs[2:])
        d_e = next(it) if self.d_flux_err is not None else None
        out = self._new(outs[0], outs[1], d_e, new_off, nan_free=self.nan_free, is_sorted=self.is_sorted)
        out.d_quality = next(it) if self.d_quality is not None else None
        out.d_cadenceno = next(it) if self.d_cadenceno is not None else None
        return out

    def remove_outliers(self, sigma=5.0, sigma_lower=None, sigma_upper=None, return_mask=False, maxiters=5):
        """``lc.remove_outliers(sigma, sigma_lower, sigma_upper)`` for every light curve (reference :1430-1556), resident:
        ``select(outlier_mask(...), invert=True)``; a cadence whose flux is not finite goes too.  ``return_mask``: also the
        mask's ``DeviceBuffer`` (bytes over the cadences of THIS batch, 1 = removed)."""
        d_m = self.outlier_mask(sigma, sigma_lower, sigma_upper, maxiters)
        out = self.select(d_m, invert=True)
        out.nan_free = True
        return (out, d_m) if return_mask else out

    def estimate_cdpp(self, transit_duration=13, savgol_window=101, savgol_polyorder=2, sigma=5.0):
        """``lc.estimate_cdpp(...)`` in ppm for every light curve (reference :1764-1833; ``lightcurve.estimate_cdpp_batch`` for
        a resident batch): flatten -> sigma clip -> ppm -> std of the ``transit_duration``-cadence running mean, all in HBM
        (``lk_savgol_trend_batch_dev``, ``lk_outlier_mask_batch_dev``, ``lk_cdpp_batch_dev``) -> float64[B] on the host: 8
        bytes per target cross PCIe.  NaN for a light curve with no cadence left."""
        if not isinstance(transit_duration, int):
            raise ValueError("transit_duration must be an integer in units number of cadences, got {}.".format(transit_duration))
        if transit_duration < 1:
            raise ValueError("transit_duration must be >= 1 cadence (got %d)" % transit_duration)
        d_tr = self.flatten_trend(savgol_window, savgol_polyorder)
        h, B, n, st = self.handle, len(self), self.n_cadences, _vp(self.stream or None)
        d_f, d_m, d_c = DeviceBuffer(h, max(n, 1) * 8), DeviceBuffer(h, max(n, 1)), DeviceBuffer(h, max(B, 1) * 8)
        _capi._check(_capi._lib.lk_flatten_apply_batch_dev(h._h, n, _vp(self.d_flux.ptr), None, _vp(d_tr.ptr), _vp(d_f.ptr), None, st))
        lo, hi, mi = _capi.clip_bounds(sigma, None, None, 5)
        _capi._check(_capi._lib.lk_outlier_mask_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(d_f.ptr), lo, hi, mi, _vp(d_m.ptr), st))
        _capi._check(_capi._lib.lk_cdpp_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(d_f.ptr), _vp(d_m.ptr), int(transit_duration),
                                                  _vp(d_c.ptr), st))
        return d_c.download(np.float64, B, stream=self.stream)

    # ---------------------------------------------------------------- fill_gaps / stitch
    def fill_gaps(self, method="gaussian_noise", by="auto", noise_std="auto", seed=0, first_target=0, stream_id=0, return_mask=False,
                  noise_mean=None):
        """``lc.fill_gaps(method="gaussian_noise")`` of lightkurve 2.x for every light curve, resident: the batch on an even grid,
        missing cadences inserted with ``quality`` 65536, ``flux_err`` linear in time between the gap's two originals and flux
        drawn from a normal distribution.  NaN-flux cadences are removed first, as the reference does; a light curve with fewer
        than 2 cadences comes back unchanged.

        ``by="time"``: the reference's loop over the sorted times, with m = median(diff(time)): a step of more than 1.2 m gets
        prev + m, prev + m + m, ... (that chain of additions: the reference's bits); the result carries no cadence numbers.
        ``by="cadenceno"``: every cadence number of [c_first, c_last], times interpolated on t - m c as the reference does
        (the originals' times are recomputed, so they may move by an ulp); this is what makes a ragged batch uniform again
        when all targets span the same cadence numbers.  ``"auto"``: by cadence number when the batch carries them.

        The flux of inserted cadence j of light curve b is ``noise_mean + noise_std * g``, g = normal j of the Philox stream
        (``seed``, target ``first_target + b``, ``stream_id``) that ``over_fitting_metric`` draws from — the reference draws
        from numpy's global generator, so the match is in distribution.  ``noise_mean``: None = nanmean(flux), or one value per
        light curve.  ``noise_std``: "std" = nanstd(flux); "cdpp" = ``estimate_cdpp() * 1e-6`` (NaN: nanstd), what the
        reference takes for a dimensionless light curve; "auto" = "cdpp" when every ``meta["NORMALIZED"]`` is true, else
        "std"; or one value per light curve.

        ``lk_fill_gaps_plan_batch_dev`` (synchronises: the new offsets come back) and ``lk_fill_gaps_batch_dev``; 32 B of
        statistics per target come to the host and 16 B go back.  ``return_mask``: also the ``DeviceBuffer`` of bytes over the
        cadences of the RESULT, 1 = inserted: ``out.select(mask, invert=True)`` gives the originals back."""
        by_cad, mode, std, mean = _fg.check_fill_gaps(method, by, self.d_cadenceno is not None, noise_std, noise_mean, self.meta)
        src = self if self.nan_free else self.remove_nans()
        if not by_cad and not src._sorted():
            raise ValueError("fill_gaps needs the light curve sorted by time")
        h, B, n, st = src.handle, len(src), src.n_cadences, _vp(src.stream or None)
        d_cad = src.d_cadenceno if by_cad else None
        d_stats, d_pos = DeviceBuffer(h, max(B, 1) * 32), DeviceBuffer(h, max(n, 1) * 4)
        new_off = np.zeros(B + 1, dtype=np.int64)
        _capi._check(_capi._lib.lk_fill_gaps_plan_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(src.d_time.ptr), _vp(src.d_flux.ptr),
                                                            _vp(d_cad.ptr if d_cad is not None else None), _vp(d_stats.ptr),
                                                            _vp(d_pos.ptr), _off_ptr(new_off), st))       # (synchronises)
        stats = d_stats.download(np.float64, 4 * B, stream=src.stream).reshape(B, 4)
        nm, ns = _fg.noise_arrays(stats, mode, std, mean, src.estimate_cdpp)
        d_nm, k1 = _upload(h, nm, src.stream)
        d_ns, k2 = _upload(h, ns, src.stream)
        nn = int(new_off[-1])
        d_t, d_f, d_m = DeviceBuffer(h, max(nn, 1) * 8), DeviceBuffer(h, max(nn, 1) * 8), DeviceBuffer(h, max(nn, 1))
        d_e = DeviceBuffer(h, max(nn, 1) * 8) if src.d_flux_err is not None else None
        d_q = DeviceBuffer(h, max(nn, 1) * 4) if src.d_quality is not None else None
        d_c = DeviceBuffer(h, max(nn, 1) * 4) if by_cad else None
        opt = lambda buf: _vp(buf.ptr if buf is not None else None)     # noqa: E731
        _capi._check(_capi._lib.lk_fill_gaps_batch_dev(
            h._h, B, _off_ptr(src.n_off), _off_ptr(new_off), _vp(src.d_time.ptr), _vp(src.d_flux.ptr), opt(src.d_flux_err),
            opt(src.d_quality), opt(d_cad), _vp(d_stats.ptr), _vp(d_pos.ptr), _vp(d_nm.ptr), _vp(d_ns.ptr), int(seed),
            int(first_target), int(stream_id), _vp(d_t.ptr), _vp(d_f.ptr), opt(d_e), opt(d_q), opt(d_c), _vp(d_m.ptr), st))
        finite = bool(np.all(np.isfinite(nm)) and np.all(np.isfinite(ns)))
        out = src._new(d_t, d_f, d_e, new_off, nan_free=finite, is_sorted=None if by_cad else True)
        out.d_quality, out.d_cadenceno = d_q, d_c
        out._keep = [k1, k2]
        out.fill_stats = stats          # m, mu, sd, n_inserted per light curve, as planned
        return (out, d_m) if return_mask else out

    def stitch(self, group=None, corrector="normalize", order="given"):
        """``LightCurveCollection(segments).stitch()`` for the light curves of this batch, resident: the light curves that
        share a value of ``group`` (int, one per light curve) become ONE target, targets numbered by first appearance;
        ``group=None``: the whole batch is one target, as a collection is.  ``corrector="normalize"`` (the reference's default
        ``corrector_func``) applies ``normalize()`` to every segment first, ``None`` leaves them as they are.  A target's
        segments are concatenated in batch order (``order="given"``: the reference's vstack, no sort) or by the time of their
        first cadence (``"start_time"``: B doubles come back through ``lk_gather_f64_dev``).  A column survives when the batch
        has it (join_type="inner").  ONE launch of ``lk_gather_segments_batch_dev`` moves every column; when the segments of
        every target already lie together in the wanted order nothing moves: the columns are shared and only the offsets
        merge.  ``meta`` is the first segment's plus ``STITCHED_FROM`` (the indices of the target's segments, in order);
        ``median_flux`` does not carry over."""
        labels = _fg.check_stitch(group, len(self), corrector, order)
        src = self.normalize() if corrector == "normalize" else self
        h, B, n, st = src.handle, len(src), src.n_cadences, _vp(src.stream or None)
        counts = np.diff(src.n_off)
        start = None
        if order == "start_time" and B:
            start = np.zeros(B)
            if n:
                _capi._check(_capi._lib.lk_gather_f64_dev(h._h, B, _off_ptr(np.minimum(src.n_off[:-1], n - 1)), _vp(src.d_time.ptr),
                                                          start.ctypes.data_as(_dp), st))
        perm, seg_off, n_off = _fg.stitch_plan(labels, counts, start)
        cols = [(src.d_time, 8), (src.d_flux, 8)]
        for buf, eb in ((src.d_flux_err, 8), (src.d_quality, 4), (src.d_cadenceno, 4)):
            if buf is not None:
                cols.append((buf, eb))
        if np.array_equal(perm, np.arange(B)):
            outs = [c for c, _eb in cols]
        else:
            outs = [DeviceBuffer(h, max(n, 1) * eb) for _c, eb in cols]
            src_start = np.ascontiguousarray(src.n_off[:-1][perm])
            dst_off = np.zeros(B + 1, dtype=np.int64)
            dst_off[1:] = np.cumsum(counts[perm])
            cin = (_vp * len(cols))(*[c.ptr for c, _eb in cols])
            cout = (_vp * len(cols))(*[c.ptr for c in outs])
            elem = np.ascontiguousarray([eb for _c, eb in cols], dtype=np.int32)
            _capi._check(_capi._lib.lk_gather_segments_batch_dev(h._h, B, _off_ptr(src_start), _off_ptr(dst_off), n, len(cols),
                                                                 elem.ctypes.data_as(_i32p), cin, cout, st))
        meta = []
        for g in range(len(seg_off) - 1):
            segs = [int(s) for s in perm[seg_off[g]:seg_off[g + 1]]]
            m = dict(src.meta[segs[0]]) if segs else {}
            m["STITCHED_FROM"] = segs
            meta.append(m)
        it = iter(outs[2:])
        d_e = next(it) if src.d_flux_err is not None else None
        out = DeviceLightCurveBatch(outs[0], outs[1], d_e, n_off, meta, src.device, src.stream, nan_free=src.nan_free)
        out.d_quality = next(it) if src.d_quality is not None else None
        out.d_cadenceno = next(it) if src.d_cadenceno is not None else None
        out._keep = list(src._keep)
        out._sorted()
        return out

    # ---------------------------------------------------------------- SFF
    def _centroid_buffer(self, c, what):
        """Centroids as a ``DeviceBuffer`` of the batch's packed layout: one as given, or a host (B, N) array / list of B
        arrays / packed array uploaded."""
        n = self.n_cadences
        if isinstance(c, DeviceBuffer):
            if c.capacity < n * 8:
                raise ValueError("%s: device buffer smaller than the batch's %d cadences" % (what, n))
            return c
        if isinstance(c, (list, tuple)):
            c = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in c]) if len(c) else np.zeros(0)
        c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
        if c.size != n:
            raise ValueError("%s needs one value per cadence of the batch (%d), got %d" % (what, n, c.size))
        buf, k = _upload(self.handle, c, self.stream)
        self._keep.append(k)
        return buf

    def sff_arclength(self, centroid_col, centroid_row, to_host=True):
        """``SFFCorrector._estimate_arclength`` per target on the device (``lk_sff_arclength_batch_dev``) -> float64[sum N] on
        the host (8 B per cadence come back), or the ``DeviceBuffer``."""
        h, B, n = self.handle, len(self), self.n_cadences
        d_c, d_r = self._centroid_buffer(centroid_col, "centroid_col"), self._centroid_buffer(centroid_row, "centroid_row")
        d_arc = DeviceBuffer(h, n * 8)
        _capi._check(_capi._lib.lk_sff_arclength_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(d_c.ptr), _vp(d_r.ptr), _vp(d_arc.ptr),
                                                           None, _vp(self.stream or None)))
        return d_arc.download(np.float64, n, stream=self.stream) if to_host else d_arc

    def sff_correct(self, centroid_col, centroid_row, windows=20, bins=5, timescale=1.5, breakindex=None, degree=3,
                    restore_trend=False, window_points=None, cadence_mask=None, sigma=5, niters=5, to_host=False,
                    max_scratch_bytes=None, diagnostics=True):
        """``SFFCorrector(lc).correct(centroid_col, centroid_row, windows, bins, timescale, breakindex, degree, restore_trend)``
        (reference correctors/sffcorrector.py) for every target of a ragged resident batch in one call of
        ``lk_sff_correct_batch_dev``: arclength, percentile knots, the block-structured design matrices and their priors, the
        regression and the component models never leave HBM.  The batch must be NaN-free with finite errors and centroids (a
        target that is not gets status 2 and NaN results; 1 = baseline shorter than 4 ``timescale``).  Centroids: host (B, N) /
        ragged lists / packed arrays, or ``DeviceBuffer``s (``DevicePixelCubeBatch.estimate_centroids(to_host=False)``).
        ``window_points``: one list of cut indices per target; None: the arclength is downloaded (8 B per cadence) and
        ``sff_window_points`` runs per target on the host — otherwise nothing but the B statuses crosses PCIe.
        ``cadence_mask``: bool over the packed cadences, True = used in the fit.  ``max_scratch_bytes``: cap of the device block
        that holds the design matrices (None: 4 GiB); groups of equal width run in chunks under it, bit-identically.
        Windows are cut BY INDEX (the reference's by-value ``np.in1d`` differs only for bit-equal arclengths in and outside a
        window).
        Returns a dict: ``lc`` (corrected ``DeviceLightCurveBatch`` sharing this batch's times), ``outlier_mask``, ``status``
        (int32[B], host), ``window_points`` and — with ``diagnostics`` — ``arclength`` / ``spline`` / ``sff``: ``DeviceBuffer``s
        (``spline`` / ``sff`` also as batches ``spline_lc`` / ``sff_lc``); ``to_host=True`` downloads them all as packed
        numpy arrays (``flux``, ``flux_err`` instead of ``lc``)."""
        from .correctors.sffcorrector import sff_window_points
        h, B, n = self.handle, len(self), self.n_cadences
        if B < 1:
            raise ValueError("sff_correct needs at least one light curve")
        if self.d_flux_err is None:
            raise ValueError("sff_correct needs flux errors")
        d_c, d_r = self._centroid_buffer(centroid_col, "centroid_col"), self._centroid_buffer(centroid_row, "centroid_row")
        if window_points is None:
            arc = self.sff_arclength(d_c, d_r)
            window_points = [sff_window_points(int(self.n_off[b + 1] - self.n_off[b]), windows, arc[self.n_off[b]:self.n_off[b + 1]],
                                               breakindex) for b in range(B)]
        win_off, wp = _capi.sff_window_arrays(window_points, self.n_off)
        idx = np.concatenate([self.n_off[:-1], self.n_off[1:] - 1]).astype(np.int64)
        ends = np.empty(2 * B, dtype=np.float64)
        _capi._check(_capi._lib.lk_gather_f64_dev(h._h, 2 * B, _off_ptr(idx), _vp(self.d_time.ptr), ends.ctypes.data_as(_dp),
                                                  _vp(self.stream or None)))
        nk = _capi.sff_n_knots(ends[:B], ends[B:], timescale)
        nbytes, _ = _capi.sff_scratch_bytes(self.n_off, nk, win_off, bins, degree, max_scratch_bytes)
        d_scr = DeviceBuffer(h, nbytes)
        d_cm = None
        if cadence_mask is not None:
            if isinstance(cadence_mask, DeviceBuffer):
                d_cm = cadence_mask
            else:
                cm = np.ascontiguousarray(cadence_mask).reshape(-1).astype(np.uint8)
                if cm.size != n:
                    raise ValueError("cadence_mask needs one entry per cadence of the batch (%d), got %d" % (n, cm.size))
                d_cm, k = _upload(h, cm, self.stream, np.uint8)
                self._keep.append(k)
        d_f, d_e, d_o = DeviceBuffer(h, n * 8), DeviceBuffer(h, n * 8), DeviceBuffer(h, n)
        d_arc = d_sp = d_sf = None
        if diagnostics:
            d_arc, d_sp, d_sf = (DeviceBuffer(h, n * 8) for _ in range(3))
        status = np.zeros(B, dtype=np.int32)

        def p(buf):
            return _vp(buf.ptr if buf is not None else None)

        _capi._check(_capi._lib.lk_sff_correct_batch_dev(
            h._h, B, _off_ptr(self.n_off), p(self.d_time), p(self.d_flux), p(self.d_flux_err), p(d_c), p(d_r), p(d_cm),
            win_off.ctypes.data_as(_i32p), wp.ctypes.data_as(_i32p), int(bins), int(degree), float(timescale),
            int(bool(restore_trend)), float(sigma), int(niters), p(d_scr), int(d_scr.capacity), p(d_f), p(d_e), p(d_o),
            status.ctypes.data_as(_i32p), p(d_arc), p(d_sp), p(d_sf), None, 0, _vp(self.stream or None)))
        wps = [np.asarray(w, dtype=np.int64) for w in window_points]
        if to_host:
            out = dict(flux=d_f.download(np.float64, n, stream=self.stream), flux_err=d_e.download(np.float64, n, stream=self.stream),
                       outlier_mask=d_o.download(np.uint8, n, stream=self.stream).astype(bool), status=status, window_points=wps)
            if diagnostics:
                for key, buf in (("arclength", d_arc), ("spline", d_sp), ("sff", d_sf)):
                    out[key] = buf.download(np.float64, n, stream=self.stream)
            return out
        lc = self._new(self.d_time, d_f, d_e, self.n_off.copy(), nan_free=bool(np.all(status == 0)), is_sorted=self.is_sorted)
        out = dict(lc=lc, outlier_mask=d_o, status=status, window_points=wps)
        if diagnostics:
            out.update(arclength=d_arc, spline=d_sp, sff=d_sf,
                       spline_lc=self._new(self.d_time, d_sp, None, self.n_off.copy(), is_sorted=self.is_sorted),
                       sff_lc=self._new(self.d_time, d_sf, None, self.n_off.copy(), is_sorted=self.is_sorted))
        return out

    # ---------------------------------------------------------------- Lomb-Scargle
    def _ls_ready(self):
        """The batch the periodogram kernels see: NaN-flux cadences dropped (LombScarglePeriodogram.from_lightcurve,
        periodogram.py:869-872), at least two cadences each."""
        src = self if self.nan_free else self.remove_nans()
        counts = np.diff(src.n_off)
        if len(counts) and counts.min() < 2:
            raise ValueError("The light curve needs at least two cadences to build a periodogram.")
        return src

    def _ls_scale(self, src, plan):
        """Device array of lightkurve's per-target psd factor (periodogram.py:865-868, 969-975), or None for 'amplitude'."""
        if plan.normalization != "psd":
            return None
        B = len(src)
        idx = np.concatenate([src.n_off[:-1], src.n_off[1:] - 1]).astype(np.int64)
        ends = np.empty(2 * B, dtype=np.float64)
        _capi._check(_capi._lib.lk_gather_f64_dev(src.handle._h, 2 * B, _off_ptr(idx), _vp(src.d_time.ptr), ends.ctypes.data_as(_dp),
                                                  _vp(src.stream or None)))
        counts = np.diff(src.n_off)
        fs = (1.0 / (ends[B:] - ends[:B])) / plan.oversample_factor * plan.unit
        scale = 2.0 / (counts * plan.oversample_factor * fs)
        d_s, k = _upload(src.handle, scale, src.stream)
        src._keep.append(k)
        return d_s

    def to_periodogram_power(self, frequency, normalization="amplitude", freq_unit=None, oversample_factor=None,
                             ls_method="fast", nterms=1, out=None, to_host=True, want_peaks=False):
        """Lomb-Scargle power of every light curve on one shared grid (``batch.lombscargle_batch`` for a resident batch:
        same plan, same kernels).  ``to_host``: float64[B, M] on the host (``out=`` a preallocated / page-locked array), else
        the ``DeviceBuffer`` holding it.  ``want_peaks``: also return float64[B, 2] (max power, argmax)."""
        plan = packed.ls_grid_plan(frequency, normalization, freq_unit, oversample_factor, ls_method, nterms)
        src = self._ls_ready()
        h, B, M, st = src.handle, len(src), len(plan.f_day), _vp(src.stream or None)
        lib = _capi._lib
        d_pow = DeviceBuffer(h, max(B * M, 1) * 8)
        d_max = DeviceBuffer(h, max(B, 1) * 8)
        d_arg = DeviceBuffer(h, max(B, 1) * 8)
        if B and M:
            d_s = self._ls_scale(src, plan)
            sp = _vp(d_s.ptr if d_s is not None else None)
            f_day, norm = plan.f_day, _capi.NORM[plan.norm]
            if plan.nterms == 1 and plan.ls_method in ("fast", "fastchi2"):
                _capi._check(lib.lk_ls_fast_peaks_lc_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(src.d_time.ptr), _vp(src.d_flux.ptr),
                                                               None, float(f_day[0]), float(f_day[1] - f_day[0]), M, 1, 1, norm, sp, 5,
                                                               _vp(d_pow.ptr), _vp(d_max.ptr), _vp(d_arg.ptr), st))
            else:
                d_trel = DeviceBuffer(h, src.n_cadences * 8)
                _capi._check(lib.lk_rebase_times_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(src.d_time.ptr), _vp(d_trel.ptr), st))
                if plan.nterms > 1 and plan.ls_method == "fastchi2":
                    _capi._check(lib.lk_ls_fastchi2_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(d_trel.ptr), _vp(src.d_flux.ptr), None,
                                                              float(f_day[0]), float(f_day[1] - f_day[0]), M, plan.nterms, 1, 1, norm,
                                                              sp, 5, _vp(d_pow.ptr), st))
                elif plan.exact is not None:
                    _capi._check(lib.lk_ls_chi2_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(d_trel.ptr), _vp(src.d_flux.ptr), None, None,
                                                          float(plan.exact[0]), float(plan.exact[1]), M, plan.nterms, 1, 1, norm, sp,
                                                          _vp(d_pow.ptr), st))
                else:
                    d_fr, k = _upload(h, f_day, src.stream)
                    src._keep.append(k)
                    _capi._check(lib.lk_ls_chi2_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(d_trel.ptr), _vp(src.d_flux.ptr), None,
                                                          _vp(d_fr.ptr), 0.0, 0.0, M, plan.nterms, 1, 1, norm, sp, _vp(d_pow.ptr), st))
                if want_peaks:
                    _capi._check(lib.lk_argmax_batch_dev(h._h, B, M, _vp(d_pow.ptr), _vp(d_max.ptr), _vp(d_arg.ptr), st))
        peaks = None
        if want_peaks:
            mx = d_max.download(np.float64, B, stream=src.stream)
            am = d_arg.download(np.int64, B, stream=src.stream)
            peaks = np.column_stack([mx, am.astype(np.float64)]) if B else np.zeros((0, 2))
        if to_host:
            if out is not None and (out.shape != (B, M) or out.dtype != np.float64 or not out.flags.c_contiguous):
                raise ValueError("out must be a C-contiguous float64 array of shape (B, M)")
            host = out if out is not None else _capi.result_empty((B, M))
            d_pow.download(np.float64, B * M, out=host.reshape(-1), stream=src.stream)
            res = host
        else:
            res = d_pow
        src._keep = []
        return (res, peaks) if want_peaks else res

    def to_periodogram_peaks(self, frequency, normalization="amplitude", freq_unit=None, oversample_factor=None):
        """(max power, argmax) per light curve of the default-method periodogram -> float64[B, 2] on the host; the spectra
        stay in HBM (``Periodogram.max_power`` / ``frequency_at_max_power``, reference periodogram.py:127-140)."""
        plan = packed.ls_grid_plan(frequency, normalization, freq_unit, oversample_factor, "fast", 1)
        if plan.ls_method != "fast":
            raise ValueError("to_periodogram_peaks needs a regular frequency grid (the reference switches to 'slow')")
        _pow, peaks = self.to_periodogram_power(frequency, normalization, freq_unit, oversample_factor, "fast", 1,
                                                to_host=False, want_peaks=True)
        return peaks

    def to_periodogram(self, frequency, normalization="psd", freq_unit=None, oversample_factor=None, ls_method="fast", nterms=1):
        """``lc.to_periodogram(frequency=..., normalization=...)`` for every light curve, the spectra left in HBM: a
        ``DevicePeriodogramBatch`` over ``to_periodogram_power(..., to_host=False)`` on the grid ``frequency`` (in
        ``freq_unit``: microhertz for 'psd', 1/d for 'amplitude' unless given) — the head of the resident chain
        ``batch.to_periodogram(f).flatten().estimate_numax()`` / ``.estimate_seismology()``."""
        plan = packed.ls_grid_plan(frequency, normalization, freq_unit, oversample_factor, ls_method, nterms)
        d_pow = self.to_periodogram_power(frequency, normalization, freq_unit, oversample_factor, ls_method, nterms, to_host=False)
        return DevicePeriodogramBatch(plan.frequency, d_pow, len(self), frequency_unit=plan.freq_unit, power_unit=plan.power_unit,
                                      device=self.device, stream=self.stream)

    def ls_model(self, frequency, nterms=1, freq_unit=None, use_flux_err=False, fit_mean=True, center_data=True, want_model=True,
                 want_residual=False, keep_mean=True, time=None):
        """``LombScarglePeriodogram.model`` before its normalisation (reference periodogram.py:991-1018 over astropy
        ``LombScargle.model``) for every light curve at its OWN frequency, resident (``lk_ls_model_batch_dev``).
        ``frequency``: a scalar or one value per target in ``freq_unit`` (default 1/d); NaN or <= 0 skips the target (status
        0).  Works on the batch the periodogram methods see (NaN flux dropped); weights are uniform, as lightkurve's, unless
        ``use_flux_err`` (1 / flux_err^2 where a target's errors are all finite).  Returns the dict of
        ``_capi.ls_model_dict`` (host arrays per target: ``frequency``, ``theta``, ``amplitude``, ``phase``, ``offset``,
        ``y_mean``, ``chi2_ref``, ``chi2_model``, ``status``) plus, resident, ``model`` (``want_model``) and ``residual``
        (``want_residual``): ``DeviceLightCurveBatch``es that share the time and flux_err buffers of the fitted batch.
        ``residual`` keeps the level ``offset`` with ``keep_mean`` (the light curve stays positive and normalised), is the
        flux bit for bit where ``status`` is not 1, and equals flux - model without ``keep_mean``.  ``time=(t_fit, m_off)``:
        ``model`` is evaluated on other times instead (host array of absolute times, target b owns
        ``t_fit[m_off[b]:m_off[b + 1]]``; ``lk_ls_model_eval_batch_dev``).  ``model``, divided by its median per target, is what
        ``LombScarglePeriodogram.model(lc.time)`` returns."""
        from .periodogram import _freq_unit_factor
        src = self._ls_ready()
        h, B, n, st = src.handle, len(src), src.n_cadences, _vp(src.stream or None)
        freq, nterms = _capi.ls_model_arguments(B, frequency, nterms)
        f_day = np.ascontiguousarray(freq / _freq_unit_factor(freq_unit if freq_unit is not None else "1/d"))
        on_time = want_model and time is None
        d_theta = DeviceBuffer(h, max(B, 1) * (2 * nterms + 1) * 8)
        d_stats = DeviceBuffer(h, max(B, 1) * _capi.LS_MODEL_NSTATS * 8)
        d_model = DeviceBuffer(h, max(n, 1) * 8) if on_time else None
        d_res = DeviceBuffer(h, max(n, 1) * 8) if want_residual else None
        d_err = src.d_flux_err if use_flux_err else None
        lib = _capi._lib
        _capi._check(lib.lk_ls_model_batch_dev(
            h._h, B, _off_ptr(src.n_off), _vp(src.d_time.ptr), _vp(src.d_flux.ptr), _vp(d_err.ptr if d_err is not None else None),
            f_day.ctypes.data_as(_dp), nterms, int(bool(fit_mean)), int(bool(center_data)), int(bool(keep_mean)), _vp(d_theta.ptr),
            _vp(d_stats.ptr), _vp(d_model.ptr if d_model is not None else None), _vp(d_res.ptr if d_res is not None else None), st))
        mdl = None
        if on_time:
            mdl = src._new(src.d_time, d_model, None, src.n_off, nan_free=True, is_sorted=src.is_sorted)
        elif want_model:
            t_fit, m_off = time
            t_fit = np.ascontiguousarray(t_fit, dtype=np.float64)
            m_off = _capi._offsets(m_off, t_fit.size)
            if m_off.size != B + 1:
                raise ValueError("time=(t_fit, m_off): m_off must hold B + 1 prefix offsets over t_fit")
            t_ref = np.zeros(B, dtype=np.float64)
            if B and n:
                _capi._check(lib.lk_gather_f64_dev(h._h, B, _off_ptr(np.minimum(src.n_off[:-1], n - 1)), _vp(src.d_time.ptr),
                                                   t_ref.ctypes.data_as(_dp), st))
            d_tf, k = _upload(h, t_fit, src.stream)
            src._keep.append(k)
            d_fit = DeviceBuffer(h, max(t_fit.size, 1) * 8)
            _capi._check(lib.lk_ls_model_eval_batch_dev(h._h, B, _off_ptr(m_off), _vp(d_tf.ptr), t_ref.ctypes.data_as(_dp),
                                                        f_day.ctypes.data_as(_dp), nterms, _vp(d_theta.ptr), _vp(d_stats.ptr),
                                                        _vp(d_fit.ptr), st))
            mdl = src._new(d_tf, d_fit, None, m_off, nan_free=True)
        theta = d_theta.download(np.float64, B * (2 * nterms + 1), stream=src.stream).reshape(B, 2 * nterms + 1)
        stats = d_stats.download(np.float64, B * _capi.LS_MODEL_NSTATS, stream=src.stream).reshape(B, _capi.LS_MODEL_NSTATS)
        src._keep = []
        out = _capi.ls_model_dict(freq, theta, stats)
        if mdl is not None:
            for m in mdl.meta:
                m["LABEL"] = "LS Model"
            out["model"] = mdl
        if want_residual:
            out["residual"] = src._new(src.d_time, d_res, src.d_flux_err, src.n_off, nan_free=True, is_sorted=src.is_sorted)
            src._carry(out["residual"])
        return out

    def prewhiten(self, frequency, n_signals=3, nterms=1, normalization="amplitude", freq_unit=None, oversample_factor=None,
                  ls_method="fast", min_power=None, use_flux_err=False):
        """Iterative prewhitening (``lc.to_periodogram()`` -> ``pg.model(lc.time)`` -> ``lc - model``, again) for every light
        curve, resident: ``n_signals`` times ``to_periodogram_power(..., to_host=False, want_peaks=True)`` on the shared grid
        ``frequency`` -> ``ls_model(frequency at each target's own peak, want_model=False, want_residual=True)``; the residual
        (level kept) is the next round's batch.  Returns (signals, residual): per round the dict of ``ls_model`` plus ``power``,
        the peak it was fitted at, strongest signal first, and the batch without every fitted signal.  A target whose peak is
        below ``min_power`` (or NaN) gets frequency NaN in that round and every later one: status 0, its flux untouched.
        ``nterms`` is the model's; the periodogram's follows ``ls_method`` as in ``to_periodogram_power``.  Per round the
        peaks and the fit parameters come down and 8 B per target go up; no column crosses PCIe."""
        if int(n_signals) < 1:
            raise ValueError("n_signals must be >= 1 (got %r)" % (n_signals,))
        plan = packed.ls_grid_plan(frequency, normalization, freq_unit, oversample_factor, ls_method, nterms)
        cur, signals = self._ls_ready(), []
        alive = np.ones(len(cur), dtype=bool)
        for _ in range(int(n_signals)):
            _pow, peaks = cur.to_periodogram_power(frequency, normalization, freq_unit, oversample_factor, ls_method, nterms,
                                                   to_host=False, want_peaks=True)
            power = peaks[:, 0]
            alive &= np.isfinite(power) if min_power is None else power >= min_power
            at = np.clip(peaks[:, 1].astype(np.int64), 0, len(plan.frequency) - 1)
            res = cur.ls_model(np.where(alive, plan.frequency[at], np.nan), nterms=nterms, freq_unit=plan.freq_unit,
                               use_flux_err=use_flux_err, want_model=False, want_residual=True)
            cur = res.pop("residual")
            res["power"] = power
            signals.append(res)
        return signals, cur

    # ---------------------------------------------------------------- BLS
    def bls(self, period, duration=None, objective="likelihood", oversample=10):
        """The seven BLS statistics of every light curve on one shared period grid, resident (``batch.bls_batch``:
        reference periodogram.py:1093-1169 over astropy ``bls_fast``) -> ``DeviceBLSResult``."""
        from .batch import _bls_options
        period, duration, objective, oversample = _bls_options(period, duration, objective, oversample)
        src = self if self.nan_free else self.remove_nans()
        counts = np.diff(src.n_off)
        if len(counts) and counts.min() < 1:
            raise ValueError("a light curve of the batch has no finite flux")
        h, B, n, nP, st = src.handle, len(src), src.n_cadences, len(period), _vp(src.stream or None)
        d_t, d_y, d_w = (DeviceBuffer(h, max(n, 1) * 8) for _ in range(3))
        d_ref = DeviceBuffer(h, max(B, 1) * 8)
        d_out = DeviceBuffer(h, max(7 * B * nP, 1) * 8)
        if B:
            lib = _capi._lib
            _capi._check(lib.lk_bls_prepare_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(src.d_time.ptr), _vp(src.d_flux.ptr),
                                                      _vp(src.d_flux_err.ptr if src.d_flux_err is not None else None), _vp(d_t.ptr),
                                                      _vp(d_y.ptr), _vp(d_w.ptr), _vp(d_ref.ptr), st))
            d_per, k = _upload(h, period, src.stream)
            _capi._check(lib.lk_bls_batch_dev(h._h, B, _off_ptr(src.n_off), _vp(d_t.ptr), _vp(d_y.ptr), _vp(d_w.ptr),
                                              period.ctypes.data_as(_dp), _vp(d_per.ptr), nP, duration.ctypes.data_as(_dp),
                                              len(duration), int(oversample), int(objective == "likelihood"), _vp(d_out.ptr), st))
            src._keep.append(k)
        return DeviceBLSResult(src, d_out, d_ref, period, duration, d_ivar=d_w)

    def bls_search(self, period, n_signals=2, duration=None, objective="likelihood", oversample=10):
        """The tutorial's planet-by-planet search (``lc[~bls.get_transit_mask(...)]`` then BLS again) for every light curve,
        resident: ``n_signals`` times ``bls(...)`` -> ``peaks()`` -> ``transit_mask(to_host=False)`` at each target's own peak ->
        ``select(mask, invert=True)``.  Returns (signals, residual): the list of the ``peaks()`` dicts, strongest signal
        first, and the batch without the transits of every signal found.  Per round only the peaks cross PCIe.  A light curve
        that has lost every cadence makes the next round's ``bls`` raise its ``ValueError``."""
        if int(n_signals) < 1:
            raise ValueError("n_signals must be >= 1 (got %r)" % (n_signals,))
        cur, signals = self, []
        for _ in range(int(n_signals)):
            res = cur.bls(period, duration, objective, oversample)
            pk = res.peaks()
            d_m = res.transit_mask(pk["period"], pk["duration"], pk["transit_time"], to_host=False)
            signals.append(pk)
            cur = res._batch.select(d_m, invert=True)
        return signals, cur

    # ---------------------------------------------------------------- fold / transit mask / bin
    def _fold_arguments(self, period, epoch_time, wrap_phase, normalize_phase):
        """(period[B], epoch_time[B], wrap_phase[B], epoch_given) as ``lk_fold_batch_dev`` takes them."""
        h, B, n = self.handle, len(self), self.n_cadences
        period = np.ascontiguousarray(np.broadcast_to(np.asarray(period, dtype=np.float64), (B,)))
        if not np.all(np.isfinite(period)) or np.any(period == 0):
            raise ValueError("period must be finite and non-zero")
        epoch_given = epoch_time is not None
        if epoch_time is None:
            epoch_time = np.zeros(B, dtype=np.float64)
            if B and n:
                first = np.ascontiguousarray(np.minimum(self.n_off[:-1], n - 1))
                _capi._check(_capi._lib.lk_gather_f64_dev(h._h, B, _off_ptr(first), _vp(self.d_time.ptr),
                                                          epoch_time.ctypes.data_as(_dp), _vp(self.stream or None)))
        epoch_time = np.ascontiguousarray(np.broadcast_to(np.asarray(epoch_time, dtype=np.float64), (B,)))
        if wrap_phase is None:
            wrap_phase = np.full(B, 0.5) if normalize_phase else period / 2.0
        wrap_phase = np.ascontiguousarray(np.broadcast_to(np.asarray(wrap_phase, dtype=np.float64), (B,)))
        return period, epoch_time, wrap_phase, epoch_given

    def fold(self, period, epoch_time=None, epoch_phase=0.0, wrap_phase=None, normalize_phase=False):
        """``lc.fold(period, epoch_time, ...)`` for every light curve (reference :1089-1214): phases + stable sort + the flux
        columns gathered into phase order, resident -> ``DeviceFoldedBatch``.  ``period`` / ``epoch_time`` / ``wrap_phase``:
        scalars or one value per light curve; ``epoch_time`` defaults to each light curve's first time."""
        h, B, n = self.handle, len(self), self.n_cadences
        period, epoch_time, wrap_phase, epoch_given = self._fold_arguments(period, epoch_time, wrap_phase, normalize_phase)
        cols = [self.d_flux] + ([self.d_flux_err] if self.d_flux_err is not None else [])
        outs = [DeviceBuffer(h, max(n, 1) * 8) for _ in cols]
        d_ph, d_ord = DeviceBuffer(h, max(n, 1) * 8), DeviceBuffer(h, max(n, 1) * 8)
        cin = (_vp * len(cols))(*[c.ptr for c in cols])
        cout = (_vp * len(cols))(*[c.ptr for c in outs])
        _capi._check(_capi._lib.lk_fold_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), period.ctypes.data_as(_dp),
                                                  epoch_time.ctypes.data_as(_dp), float(epoch_phase), wrap_phase.ctypes.data_as(_dp),
                                                  int(bool(normalize_phase)), len(cols), cin, cout, _vp(d_ph.ptr), _vp(d_ord.ptr),
                                                  _vp(self.stream or None)))
        return DeviceFoldedBatch(self, d_ph, outs[0], outs[1] if len(outs) > 1 else None, d_ord, period, epoch_time,
                                 epoch_given=epoch_given, epoch_phase=epoch_phase, wrap_phase=wrap_phase,
                                 normalize_phase=normalize_phase)

    def _fold_bin_plan(self, period, epoch_time, epoch_given, epoch_phase, wrap_phase, normalize_phase, count_from=None):
        """``lk_fold_bin_plan_batch_dev``: float64[B, 8] on the host (smallest / largest phase, count, has_err, smallest cycle,
        max |flux|, max |flux_err|, flux range) from one pass over the unfolded cadences; 64 B per target cross PCIe."""
        B = len(self)
        plan = np.zeros((max(B, 1), _fb.NPLAN), dtype=np.float64)
        cf = None if count_from is None else np.ascontiguousarray(count_from, dtype=np.float64)
        _capi._check(_capi._lib.lk_fold_bin_plan_batch_dev(
            self.handle._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), _vp(self.d_flux.ptr),
            _vp(self.d_flux_err.ptr if self.d_flux_err is not None else None), period.ctypes.data_as(_dp),
            epoch_time.ctypes.data_as(_dp), int(epoch_given), float(epoch_phase), wrap_phase.ctypes.data_as(_dp),
            int(bool(normalize_phase)), None if cf is None else cf.ctypes.data_as(_dp), plan.ctypes.data_as(_dp),
            _vp(self.stream or None)))
        return plan[:B]

    def fold_bin(self, period, epoch_time=None, epoch_phase=0.0, wrap_phase=None, normalize_phase=False, time_bin_size=None,
                 time_bin_start=None, n_bins=None, bins=None, aggregate_func="mean", which="all"):
        """``lc.fold(period, epoch_time, ...).bin(...)`` for every light curve, FUSED: no sort, no folded copy, about 200
        numbers per target instead of four n-sized columns -> ``DevicePhaseCurveBatch``.  The fold arguments are ``fold``'s, the
        bin arguments ``DeviceFoldedBatch.bin``'s; the result has the layout, counts and NaN pattern of
        ``self.fold(...).bin(...)`` and its values within 1e-9 relative (its sums are exact integer sums of the addends
        rounded to 2^-63 n max|x|: bitwise reproducible, independent of the other light curves).  ``aggregate_func="mean"``
        only: a median needs the sorted slots, use ``fold(...).bin(aggregate_func="median")``.

        Two launches: a pre-kernel streams the cadences once and returns 64 B per target (phase range, smallest cycle,
        scales), from which the host sizes the output and forms every target's edges; the main kernel (one workgroup per
        target) streams them again and accumulates per bin in LDS — up to 1024 bins per target, more go through a slab in
        device memory."""
        aggregate_func, which_code = _fb.check_bin_arguments(time_bin_size, n_bins, bins, aggregate_func, which)
        if aggregate_func != "mean":
            raise ValueError("the fused fold_bin supports aggregate_func='mean' only: use fold(...).bin(aggregate_func='median')")
        h, B = self.handle, len(self)
        period, epoch_time, wrap_phase, epoch_given = self._fold_arguments(period, epoch_time, wrap_phase, normalize_phase)
        plan = self._fold_bin_plan(period, epoch_time, epoch_given, epoch_phase, wrap_phase, normalize_phase,
                                   _fb.count_from(time_bin_start, bins, B))
        lay = _fb.phase_bin_layout(np.diff(self.n_off), plan, time_bin_size, time_bin_start, n_bins, bins)
        cyc_epoch = epoch_time if epoch_given else np.ascontiguousarray(plan[:, 0])
        out = DevicePhaseCurveBatch._empty(self, lay)
        _capi._check(_capi._lib.lk_fold_bin_batch_dev(
            h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), _vp(self.d_flux.ptr),
            _vp(self.d_flux_err.ptr if self.d_flux_err is not None else None), period.ctypes.data_as(_dp),
            epoch_time.ctypes.data_as(_dp), float(epoch_phase), wrap_phase.ctypes.data_as(_dp), int(bool(normalize_phase)),
            cyc_epoch.ctypes.data_as(_dp), np.ascontiguousarray(plan).ctypes.data_as(_dp), which_code, _off_ptr(lay["bin_off"]),
            lay["start"].ctypes.data_as(_dp), lay["size_sec"].ctypes.data_as(_dp), lay["edges"].ctypes.data_as(_dp),
            _vp(out.d_phase.ptr), _vp(out.d_flux.ptr), _vp(out.d_flux_err.ptr), _vp(out.d_count.ptr), _vp(self.stream or None)))
        out._parent = self
        return out

    def river(self, period, epoch_time=None, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5, method="mean", bins=None,
              max_output_mb=4096):
        """River diagrams: per light curve an image of shape (cycles, phase bins), the data behind ``LightCurve.plot_river`` of
        lightkurve 2.x -> ``DeviceRiverBatch`` (plotting itself stays out of scope).  The one view that keeps the cycles apart:
        is the signal in every transit, does it drift in phase, does one stretch of data carry the detection.

        ``y = flux / nanmedian(flux)``; the phase is ``fold(period, epoch_time, normalize_phase=True)``'s (the same bits), the
        row ``FoldedLightCurve.cycle`` (rows of cycles without a cadence exist and are empty); ``n_bins = bins`` or
        ``int(period / nanmedian(diff(time)) * (maximum_phase - minimum_phase) / bin_points)``; edges
        ``np.linspace(minimum_phase, maximum_phase, n_bins + 1)``, a cadence is in column j when ``edges[j] < phase <=
        edges[j+1]`` (a phase equal to ``edges[0]``, -0.5 in particular, is in none) and takes part when its y is finite.
        ``method``: ``"mean"`` / ``"median"`` of the cell's y, or ``"sigma"`` = ``(mean - 1) / sqrt(nansum((flux_err /
        nanmedian(flux))^2))`` (needs ``flux_err``).  A cell nobody takes part in holds NaN, count 0.  ``period`` / ``epoch_time``
        (default: each light curve's first time) / ``bins``: a scalar or one value per light curve.

        Deviations from the reference, on purpose: rows are this project's cycles, cut at phase +-0.5 of the given epoch (the
        reference cuts at ``time % period``, so a row boundary can fall inside a transit); with ``bin_points == 1`` every cell
        is still aggregated (the reference takes the cell's first cadence; equal when a cell holds one); ``sigma`` is the
        reference's expression, not divided by the count.

        No exception per light curve: ``status`` 1 fewer than two cadences or no finite flux, 2 times decreasing or not finite,
        3 median flux not finite or zero or median time step not positive, 4 ``n_bins < 1``; such a light curve has no cell.
        ``ValueError`` for bad arguments and when the images exceed ``max_output_mb`` MiB.  Two launches: a plan kernel (72 B
        per target to the host) and the image kernel, one workgroup per tile of rows; medians are exact, means within
        n 2^-63 max|y| (exact integer sums): a light curve's image has the same bits alone and in any batch."""
        h, B = self.handle, len(self)
        period, bins, code = _rv.check_arguments(B, period, bin_points, minimum_phase, maximum_phase, method, bins,
                                                 has_err=self.d_flux_err is not None)
        epoch_given = epoch_time is not None
        epoch = np.ascontiguousarray(np.broadcast_to(np.asarray(epoch_time if epoch_given else 0.0, dtype=np.float64), (B,)))
        d_err = _vp(self.d_flux_err.ptr if self.d_flux_err is not None else None)
        plan = np.zeros((max(B, 1), _rv.NPLAN), dtype=np.float64)
        _capi._check(_capi._lib.lk_river_plan_batch_dev(
            h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), _vp(self.d_flux.ptr), d_err, period.ctypes.data_as(_dp),
            epoch.ctypes.data_as(_dp), int(epoch_given), plan.ctypes.data_as(_dp), _vp(self.stream or None)))
        plan = plan[:B]
        lay = _rv.layout(np.diff(self.n_off), plan, period, bin_points, minimum_phase, maximum_phase, bins, max_output_mb)
        if not epoch_given:
            epoch = np.ascontiguousarray(plan[:, 6])
        ncell = int(lay["cell_off"][-1])
        d_river, d_count = DeviceBuffer(h, max(ncell, 1) * 8), DeviceBuffer(h, max(ncell, 1) * 4)
        d_route = DeviceBuffer(h, max(B, 1) * 4)
        _capi._check(_capi._lib.lk_river_batch_dev(
            h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), _vp(self.d_flux.ptr), d_err, period.ctypes.data_as(_dp),
            epoch.ctypes.data_as(_dp), np.ascontiguousarray(plan).ctypes.data_as(_dp), code, lay["n_bins"].ctypes.data_as(_i32p),
            lay["n_cycles"].ctypes.data_as(_i32p), _off_ptr(lay["cell_off"]), lay["edges"].ctypes.data_as(_dp), _vp(d_river.ptr),
            _vp(d_count.ptr), _vp(d_route.ptr), _vp(self.stream or None)))
        out = DeviceRiverBatch(h, self.stream, d_river, d_count, d_route, lay, period, epoch, method, self.meta)
        out._parent = self
        return out

    def create_transit_mask(self, period, transit_time, duration, planet_off=None, to_host=True):
        """In-transit flags over all cadences of the batch (reference :2967-3037) -> bool array on the host, or the
        ``DeviceBuffer`` of bytes (usable as ``flatten(mask=...)``) with ``to_host=False``."""
        h, B, n = self.handle, len(self), self.n_cadences
        period, duration, transit_time = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64)
                                          for a in (period, duration, transit_time))
        if not (period.shape == duration.shape == transit_time.shape):
            raise ValueError("period, duration, and transit_time must have the same number of values.")
        if planet_off is None:
            k = period.size
            period, duration, transit_time = (np.tile(a, B) for a in (period, duration, transit_time))
            planet_off = np.arange(B + 1, dtype=np.int32) * k
        planet_off = np.ascontiguousarray(planet_off, dtype=np.int32)
        if planet_off.shape != (B + 1,) or planet_off[0] != 0 or planet_off[-1] != period.size:
            raise ValueError("planet_off must be B + 1 prefix offsets over the planet arrays")
        d_m = DeviceBuffer(h, max(n, 1))
        _capi._check(_capi._lib.lk_transit_mask_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr),
                                                          planet_off.ctypes.data_as(_i32p), period.ctypes.data_as(_dp),
                                                          duration.ctypes.data_as(_dp), transit_time.ctypes.data_as(_dp),
                                                          _vp(d_m.ptr), _vp(self.stream or None)))
        if not to_host:
            return d_m
        return d_m.download(np.uint8, n, stream=self.stream).astype(bool)

    def bin(self, time_bin_size=0.5, time_bin_start=None):
        """Equal-width time bins (reference :1558-1763 with ``time_bin_size`` in days), resident: nanmean flux, rms flux_err."""
        h, B, n, st = self.handle, len(self), self.n_cadences, _vp(self.stream or None)
        size_sec = float(time_bin_size) * 86400.0
        if not size_sec > 0:
            raise ValueError("time_bin_size must be positive")
        if not self._sorted():
            raise ValueError("bin needs the light curve sorted by time")
        idx = np.concatenate([self.n_off[:-1], np.maximum(self.n_off[1:] - 1, 0)]).astype(np.int64)
        ends = np.zeros(2 * B, dtype=np.float64)
        if n:
            _capi._check(_capi._lib.lk_gather_f64_dev(h._h, 2 * B, _off_ptr(np.minimum(idx, n - 1)), _vp(self.d_time.ptr),
                                                      ends.ctypes.data_as(_dp), st))
        counts = np.diff(self.n_off)
        fin = np.zeros(max(B, 1), dtype=np.int64)
        if self.d_flux_err is not None and B:
            _capi._check(_capi._lib.lk_segment_probe_batch_dev(h._h, B, _off_ptr(self.n_off), None, _vp(self.d_flux_err.ptr), None,
                                                               _off_ptr(fin), st))
        first, last = ends[:B], ends[B:]
        start = first.copy() if time_bin_start is None else np.broadcast_to(np.asarray(time_bin_start, float), (B,)).copy()
        start[counts == 0] = 0.0
        nb = np.where(counts > 0, np.maximum(0, np.ceil((last - start) * 86400.0 / size_sec)), 0).astype(np.int64)
        has_err = (fin[:B] > 0).astype(np.uint8)
        bin_off = np.zeros(B + 1, dtype=np.int64)
        bin_off[1:] = np.cumsum(nb)
        edges = np.cumsum(np.hstack([0.0, np.repeat(size_sec, int(nb.max()) if B else 0)]))
        nbt = int(bin_off[-1])
        d_t, d_f, d_e = (DeviceBuffer(h, max(nbt, 1) * 8) for _ in range(3))
        u8p = ctypes.POINTER(ctypes.c_uint8)
        _capi._check(_capi._lib.lk_bin_batch_dev(h._h, B, _off_ptr(self.n_off), _vp(self.d_time.ptr), _vp(self.d_flux.ptr),
                                                 _vp(self.d_flux_err.ptr if self.d_flux_err is not None else None), _off_ptr(bin_off),
                                                 start.ctypes.data_as(_dp), edges.ctypes.data_as(_dp), int(edges.size), size_sec,
                                                 has_err.ctypes.data_as(u8p), _vp(d_t.ptr), _vp(d_f.ptr), _vp(d_e.ptr), st))
        return self._new(d_t, d_f, d_e, bin_off, nan_free=False, is_sorted=True)


class DeviceFoldedBatch(object):
    """Folded light curves in HBM: phase (sorted), flux / flux_err in phase order, ``order`` (index of the cadence, relative to
    its light curve, at each sorted slot) — the reference's ``FoldedLightCurve`` for a batch: ``cycle`` / ``odd_mask`` /
    ``even_mask`` per slot and ``bin`` by phase."""

    def __init__(self, parent, d_phase, d_flux, d_flux_err, d_order, period, epoch_time, epoch_given=True, epoch_phase=0.0,
                 wrap_phase=None, normalize_phase=False):
        self.handle, self.stream, self.n_off = parent.handle, parent.stream, parent.n_off
        self.d_phase, self.d_flux, self.d_flux_err, self.d_order = d_phase, d_flux, d_flux_err, d_order
        self.period, self.epoch_time = period, epoch_time
        self.epoch_given = bool(epoch_given)     # False: fold() took each light curve's first time (the cycle's epoch differs)
        self.epoch_phase, self.normalize_phase = float(epoch_phase), bool(normalize_phase)
        if wrap_phase is None:
            wrap_phase = np.full(len(period), 0.5) if normalize_phase else np.asarray(period) / 2.0
        self.wrap_phase = np.ascontiguousarray(wrap_phase, dtype=np.float64)
        self.meta = parent.meta
        self._parent = parent            # (keeps the unfolded columns alive while the fold kernels may still read them)
        self._plan0 = None

    def __len__(self):
        return len(self.n_off) - 1

    def to_host(self):
        """-> dict(phase, flux, flux_err, order, n_off) of host arrays."""
        n = int(self.n_off[-1])
        return dict(phase=self.d_phase.download(np.float64, n, stream=self.stream),
                    flux=self.d_flux.download(np.float64, n, stream=self.stream),
                    flux_err=None if self.d_flux_err is None else self.d_flux_err.download(np.float64, n, stream=self.stream),
                    order=self.d_order.download(np.int64, n, stream=self.stream), n_off=self.n_off.copy())

    # ---------------------------------------------------------------- cycle / odd / even
    def _plan(self, count_from=None):
        if count_from is None and self._plan0 is not None:
            return self._plan0
        plan = self._parent._fold_bin_plan(self.period, self.epoch_time, self.epoch_given, self.epoch_phase, self.wrap_phase,
                                           self.normalize_phase, count_from)
        if count_from is None:
            self._plan0 = plan
        return plan

    def _cycle_buffers(self, want_cycle, want_odd, want_even):
        h, B, n = self.handle, len(self), int(self.n_off[-1])
        plan = self._plan()
        # the reference's rule (lightcurve.py:178-182): the epoch given to fold(), else the smallest folded phase
        cyc_epoch = self.epoch_time if self.epoch_given else np.ascontiguousarray(plan[:, 0])
        cyc_min = np.ascontiguousarray(plan[:, 4])
        d_c = DeviceBuffer(h, max(n, 1) * 8) if want_cycle else None
        d_o = DeviceBuffer(h, max(n, 1)) if want_odd else None
        d_e = DeviceBuffer(h, max(n, 1)) if want_even else None
        _capi._check(_capi._lib.lk_fold_cycle_batch_dev(
            h._h, B, _off_ptr(self.n_off), _vp(self._parent.d_time.ptr), _vp(self.d_order.ptr), self.period.ctypes.data_as(_dp),
            cyc_epoch.ctypes.data_as(_dp), cyc_min.ctypes.data_as(_dp), _vp(d_c.ptr if d_c else None),
            _vp(d_o.ptr if d_o else None), _vp(d_e.ptr if d_e else None), _vp(self.stream or None)))
        return d_c, d_o, d_e

    def cycle(self, to_host=True):
        """``FoldedLightCurve.cycle`` per slot, in phase order: floor((time_original - (e - P/2)) / P) minus its minimum over
        the light curve, with e the ``epoch_time`` given to ``fold`` or, without one, the smallest folded phase (the
        reference's rule).  int64 on the host, or the ``DeviceBuffer`` with ``to_host=False``."""
        d_c = self._cycle_buffers(True, False, False)[0]
        return d_c.download(np.int64, int(self.n_off[-1]), stream=self.stream) if to_host else d_c

    def odd_mask(self, to_host=True):
        """``cycle % 2 == 1`` per slot -> bool array, or the ``DeviceBuffer`` of bytes (usable with ``select`` /
        ``flatten(mask=)``-style calls on a batch in phase order) with ``to_host=False``."""
        d_m = self._cycle_buffers(False, True, False)[1]
        return d_m.download(np.uint8, int(self.n_off[-1]), stream=self.stream).astype(bool) if to_host else d_m

    def even_mask(self, to_host=True):
        """``cycle % 2 == 0`` per slot (see ``odd_mask``)."""
        d_m = self._cycle_buffers(False, False, True)[2]
        return d_m.download(np.uint8, int(self.n_off[-1]), stream=self.stream).astype(bool) if to_host else d_m

    def as_lightcurves(self):
        """The folded columns as a ``DeviceLightCurveBatch`` whose time is the phase (no copy): what ``select(mask)`` with an
        ``odd_mask(to_host=False)`` / ``even_mask(to_host=False)`` works on."""
        out = self._parent._new(self.d_phase, self.d_flux, self.d_flux_err, self.n_off, nan_free=False, is_sorted=True)
        out._folded = self               # (keeps the folded buffers' owner alive)
        return out

    # ---------------------------------------------------------------- bin by phase
    def bin(self, time_bin_size=None, time_bin_start=None, n_bins=None, bins=None, aggregate_func="mean", which="all"):
        """``FoldedLightCurve.bin`` for every light curve -> ``DevicePhaseCurveBatch``.  ``LightCurve.bin``'s semantics
        (reference :1558-1763 over astropy 4.3.1 ``aggregate_downsample``) on the phase column: relative time
        ``(phase - start) * 86400``, edges = numpy's running sum of the bin size, slot in bin k when ``edges[k] < r <=
        edges[k+1]`` (``r == 0``: bin 0) and ``r < edges[n_bins]``.

        ``time_bin_size`` (default 0.5, in the units of the phase) and ``time_bin_start`` (default: each light curve's
        smallest phase): a scalar or one value per light curve, the edges are each light curve's own running sum.
        ``n_bins`` defaults to ``ceil(r_last / size)`` (a last slot exactly on the last edge is dropped, as in the
        reference).  ``bins=int`` is the reference's v1-compatibility form: ``time_bin_size = (phase_last - start) * i /
        ((i - 1) * bins)`` with i the number of slots whose phase is >= start - 1 ns (``ValueError`` when i < 2 or together with
        ``time_bin_size`` / ``n_bins``); the formula as written here is the contract (the reference's source was not at hand).

        ``aggregate_func``: "mean" (nanmean) or "median" (``np.nanmedian`` of the bin's flux).  Stated deviation: ``flux_err``
        is the rms of the bin's errors — ``sqrt(nansum(err^2) / #finite)`` — or, for a light curve without a finite error, the
        nanstd of the bin's flux, for BOTH aggregates.  ``which``: "all", "odd" or "even" restricts the slots by the parity of
        ``cycle()``; the layout (start, size, n_bins) is always taken from all slots, so the odd and the even curve of a
        light curve sit on the same bins.  ``count`` is the number of slots of the bin that took part; a bin with none is NaN."""
        aggregate_func, which_code = _fb.check_bin_arguments(time_bin_size, n_bins, bins, aggregate_func, which)
        h, B = self.handle, len(self)
        plan = self._plan(_fb.count_from(time_bin_start, bins, B))
        lay = _fb.phase_bin_layout(np.diff(self.n_off), plan, time_bin_size, time_bin_start, n_bins, bins)
        d_sel = self._cycle_buffers(False, True, False)[1] if which_code else None
        has_err = (plan[:, 3] > 0).astype(np.uint8) if self.d_flux_err is not None else np.zeros(B, dtype=np.uint8)
        has_err = np.ascontiguousarray(has_err if B else np.zeros(1, dtype=np.uint8))
        out = DevicePhaseCurveBatch._empty(self, lay)
        _capi._check(_capi._lib.lk_phase_bin_batch_dev(
            h._h, B, _off_ptr(self.n_off), _vp(self.d_phase.ptr), _vp(self.d_flux.ptr),
            _vp(self.d_flux_err.ptr if self.d_flux_err is not None else None), _vp(d_sel.ptr if d_sel is not None else None),
            1 if which_code == 1 else 0, _off_ptr(lay["bin_off"]), lay["start"].ctypes.data_as(_dp),
            lay["size_sec"].ctypes.data_as(_dp), lay["edges"].ctypes.data_as(_dp),
            has_err.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), int(aggregate_func == "median"), _vp(out.d_phase.ptr),
            _vp(out.d_flux.ptr), _vp(out.d_flux_err.ptr), _vp(out.d_count.ptr), _vp(self.stream or None)))
        out._parent = (self, d_sel)
        return out


class DevicePhaseCurveBatch(object):
    """Phase-binned folded light curves in HBM: ``d_phase`` (bin centres), ``d_flux``, ``d_flux_err`` (float64) and ``d_count``
    (int32 cadences per bin), target b's bins at ``[bin_off[b], bin_off[b + 1])`` (``bin_off``: host, B + 1).  ``start`` /
    ``time_bin_size`` (host, per target) are the layout the bins were formed on."""

    def __init__(self, handle, stream, d_phase, d_flux, d_flux_err, d_count, bin_off, start, time_bin_size, meta=None):
        self.handle, self.stream = handle, stream
        self.d_phase, self.d_flux, self.d_flux_err, self.d_count = d_phase, d_flux, d_flux_err, d_count
        self.bin_off = np.ascontiguousarray(bin_off, dtype=np.int64)
        self.start, self.time_bin_size = start, time_bin_size
        self.meta = meta
        self._parent = None              # (keeps the inputs alive while the kernels may still read them)

    @classmethod
    def _empty(cls, src, lay):
        nbt = int(lay["bin_off"][-1])
        d_p, d_f, d_e = (DeviceBuffer(src.handle, max(nbt, 1) * 8) for _ in range(3))
        d_c = DeviceBuffer(src.handle, max(nbt, 1) * 4)
        return cls(src.handle, src.stream, d_p, d_f, d_e, d_c, lay["bin_off"], lay["start"], lay["size"], src.meta)

    def __len__(self):
        return len(self.bin_off) - 1

    @property
    def n_bins(self):
        return np.diff(self.bin_off)

    def to_host(self):
        """-> dict(phase, flux, flux_err, count, bin_off) of host arrays."""
        nbt = int(self.bin_off[-1])
        return dict(phase=self.d_phase.download(np.float64, nbt, stream=self.stream),
                    flux=self.d_flux.download(np.float64, nbt, stream=self.stream),
                    flux_err=self.d_flux_err.download(np.float64, nbt, stream=self.stream),
                    count=self.d_count.download(np.int32, nbt, stream=self.stream), bin_off=self.bin_off.copy())


class DeviceRiverBatch(object):
    """River diagrams in HBM: ``d_river`` (float64) and ``d_count`` (int32 cadences per cell), target b's cells at
    ``[cell_off[b], cell_off[b + 1])``, row-major as ``(n_cycles[b], n_bins[b])``.  Host arrays per target: ``status`` (0 ok; a
    non-zero status has no cell), ``n_cycles``, ``n_bins``, ``cycle_min`` (the cycle number of row 0) and ``edges`` (target b's
    ``n_bins[b] + 1`` phase edges at ``edge_off[b]``: ``edges_of(b)``); ``cell_off`` (B + 1)."""

    def __init__(self, handle, stream, d_river, d_count, d_route, lay, period, epoch_time, method, meta=None):
        self.handle, self.stream = handle, stream
        self.d_river, self.d_count, self._d_route = d_river, d_count, d_route
        self.cell_off, self.n_cycles, self.n_bins = lay["cell_off"], lay["n_cycles"], lay["n_bins"]
        self.status, self.edges, self.edge_off, self.cycle_min = lay["status"], lay["edges"], lay["edge_off"], lay["cycle_min"]
        self.period, self.epoch_time, self.method = period, epoch_time, method
        self.meta = meta
        self._parent = None              # (keeps the inputs alive while the kernels may still read them)

    def __len__(self):
        return len(self.cell_off) - 1

    def edges_of(self, b):
        """The ``n_bins[b] + 1`` phase edges of target b (empty for a non-zero status)."""
        return self.edges[self.edge_off[b]:self.edge_off[b + 1]] if self.status[b] == 0 else np.zeros(0)

    def routes(self):
        """int32[B]: per target the OR of its tiles' ``river.ROUTE_*`` bits (which kernel routes served it)."""
        return self._d_route.download(np.int32, len(self), stream=self.stream)

    def to_host(self):
        """-> dict(river, count: lists of per-target (n_cycles_b, n_bins_b) arrays; n_cycles, n_bins, status, cell_off, edges,
        edge_off, cycle_min)."""
        ncell = int(self.cell_off[-1])
        lay = dict(cell_off=self.cell_off, n_cycles=self.n_cycles, n_bins=self.n_bins)
        river = self.d_river.download(np.float64, ncell, stream=self.stream)
        count = self.d_count.download(np.int32, ncell, stream=self.stream)
        return dict(river=_rv.split(river, lay), count=_rv.split(count, lay), n_cycles=self.n_cycles.copy(), n_bins=self.n_bins.copy(),
                    status=self.status.copy(), cell_off=self.cell_off.copy(), edges=self.edges.copy(), edge_off=self.edge_off.copy(),
                    cycle_min=self.cycle_min.copy())


class DeviceBLSResult(object):
    """out7[7, B, nP] in HBM (``_capi.BLS_FIELDS`` order; transit_time relative to ``t_ref``, the reference's
    ``min(t)`` per light curve) + what a pipeline keeps of it."""

    def __init__(self, batch, d_out7, d_t_ref, period, duration, d_ivar=None):
        self.handle, self.stream, self.B = batch.handle, batch.stream, len(batch)
        self.d_out7, self.d_t_ref, self.period, self.duration = d_out7, d_t_ref, period, duration
        self._batch = batch              # the NaN-free batch the search ran on
        self.d_ivar = d_ivar             # its prepared ivar (lk_bls_prepare_batch_dev); None: ones

    def to_host(self):
        """float64[B, 7, nP] as ``batch.bls_batch`` returns it (transit_time absolute, like the reference)."""
        B, nP = self.B, len(self.period)
        raw = self.d_out7.download(np.float64, 7 * B * nP, stream=self.stream).reshape(7, B, nP)
        t_ref = self.d_t_ref.download(np.float64, B, stream=self.stream)
        out = np.ascontiguousarray(np.transpose(raw, (1, 0, 2)))
        out[:, 4, :] += t_ref[:, None]
        return out

    def peaks(self):
        """Per light curve, at the maximum of the power: dict(max_power, argmax, period, transit_time (absolute), duration,
        depth) — ``BoxLeastSquaresPeriodogram.*_at_max_power`` (reference periodogram.py:1229-1260); 48 B per target cross PCIe."""
        h, B, nP, st = self.handle, self.B, len(self.period), _vp(self.stream or None)
        d_max, d_arg = DeviceBuffer(h, max(B, 1) * 8), DeviceBuffer(h, max(B, 1) * 8)
        if B == 0:
            z = np.zeros(0)
            return dict(max_power=z, argmax=z.astype(np.int64), period=z, transit_time=z, duration=z, depth=z)
        _capi._check(_capi._lib.lk_argmax_batch_dev(h._h, B, nP, _vp(self.d_out7.ptr), _vp(d_max.ptr), _vp(d_arg.ptr), st))
        mx = d_max.download(np.float64, B, stream=self.stream)
        am = d_arg.download(np.int64, B, stream=self.stream)
        a = np.clip(am, 0, nP - 1)
        rows = {"depth": 1, "duration": 3, "transit_time": 4}
        idx = np.concatenate([r * B * nP + np.arange(B) * nP + a for r in rows.values()]).astype(np.int64)
        vals = np.empty(idx.size, dtype=np.float64)
        _capi._check(_capi._lib.lk_gather_f64_dev(h._h, idx.size, _off_ptr(idx), _vp(self.d_out7.ptr), vals.ctypes.data_as(_dp), st))
        t_ref = self.d_t_ref.download(np.float64, B, stream=self.stream)
        got = {k: vals[i * B:(i + 1) * B] for i, k in enumerate(rows)}
        return dict(max_power=mx, argmax=am, period=self.period[a], transit_time=got["transit_time"] + t_ref,
                    duration=got["duration"], depth=got["depth"])

    # ---------------------------------------------------------------- vetting: compute_stats / model / mask
    def _box(self, period, duration, transit_time):
        """(period, duration, transit_time)[B]: each a scalar or one value per target; None = the value at the peak."""
        if period is None or duration is None or transit_time is None:
            pk = self.peaks()
            period = pk["period"] if period is None else period
            duration = pk["duration"] if duration is None else duration
            transit_time = pk["transit_time"] if transit_time is None else transit_time
        return _capi.bls_stats_arguments(self.B, period, duration, transit_time)

    def _stats(self, period, duration, transit_time, want_model, tr_off=None):
        src = self._batch
        if not src._sorted():
            raise ValueError("compute_stats / transit_model need every light curve sorted by time")
        period, duration, transit_time = self._box(period, duration, transit_time)
        h, B, n, st = self.handle, self.B, src.n_cadences, _vp(self.stream or None)
        idx = np.concatenate([src.n_off[:-1], np.maximum(src.n_off[1:] - 1, 0)]).astype(np.int64)
        ends = np.zeros(2 * B, dtype=np.float64)
        if B and n:
            _capi._check(_capi._lib.lk_gather_f64_dev(h._h, 2 * B, _off_ptr(np.minimum(idx, n - 1)), _vp(src.d_time.ptr),
                                                      ends.ctypes.data_as(_dp), st))
        t_first = ends[:B]
        if tr_off is None:
            tr_off = _capi.bls_stats_slots(t_first, ends[B:], period)
        tr_off = np.ascontiguousarray(tr_off, dtype=np.int64)
        ntr = int(tr_off[-1])
        d_stats = DeviceBuffer(h, max(B, 1) * _capi.BLS_NSTATS * 8)
        d_first, d_n = DeviceBuffer(h, max(B, 1) * 4), DeviceBuffer(h, max(B, 1) * 4)
        d_cnt, d_ll = DeviceBuffer(h, max(ntr, 1) * 4), DeviceBuffer(h, max(ntr, 1) * 8)
        d_model = DeviceBuffer(h, max(n, 1) * 8) if want_model else None
        _capi._check(_capi._lib.lk_bls_stats_batch_dev(
            h._h, B, _off_ptr(src.n_off), _vp(src.d_time.ptr), _vp(src.d_flux.ptr), _vp(self.d_ivar.ptr if self.d_ivar is not None else None),
            period.ctypes.data_as(_dp), duration.ctypes.data_as(_dp), transit_time.ctypes.data_as(_dp), _off_ptr(tr_off),
            _vp(d_stats.ptr), _vp(d_first.ptr), _vp(d_n.ptr), _vp(d_cnt.ptr), _vp(d_ll.ptr),
            _vp(d_model.ptr if d_model is not None else None), st))
        return dict(period=period, transit_time=transit_time, t_first=t_first, tr_off=tr_off, d_stats=d_stats, d_first=d_first,
                    d_n=d_n, d_cnt=d_cnt, d_ll=d_ll, d_model=d_model)

    def compute_stats(self, period=None, duration=None, transit_time=None):
        """``BoxLeastSquaresPeriodogram.compute_stats`` (reference periodogram.py:1194-1229 over astropy compute_stats) of one
        box per target, on the resident batch (``lk_bls_stats_batch_dev``).  ``period`` / ``duration`` / ``transit_time``
        (absolute): a scalar or one value per target; None = the value at the target's maximum power (``peaks()``).
        Returns a dict of host arrays: ``depth`` / ``depth_phased`` / ``depth_half`` / ``depth_odd`` / ``depth_even``
        [B, 2] (value, error), ``harmonic_amplitude`` / ``harmonic_delta_log_likelihood`` [B], ``n_transits`` [B],
        ``transit_off`` [B + 1] and the packed ``transit_times`` (absolute) / ``per_transit_count`` /
        ``per_transit_log_likelihood``: target b's slice ``[transit_off[b]:transit_off[b + 1]]`` is the array astropy's dict
        holds.  A target without an in-transit cadence has ``n_transits`` 0 (astropy raises).  The light curves must be sorted
        by time (``ValueError``)."""
        r = self._stats(period, duration, transit_time, False)
        B, ntr = self.B, int(r["tr_off"][-1])
        stats = r["d_stats"].download(np.float64, B * _capi.BLS_NSTATS, stream=self.stream).reshape(B, _capi.BLS_NSTATS)
        tr_first = r["d_first"].download(np.int32, B, stream=self.stream)
        tr_n = r["d_n"].download(np.int32, B, stream=self.stream)
        tr_count = r["d_cnt"].download(np.int32, ntr, stream=self.stream)
        tr_ll = r["d_ll"].download(np.float64, ntr, stream=self.stream)
        return _capi.bls_stats_dict(stats, tr_first, tr_n, r["tr_off"], tr_count, tr_ll, r["period"], r["transit_time"], r["t_first"])

    def transit_model(self, period=None, duration=None, transit_time=None):
        """``BoxLeastSquaresPeriodogram.get_transit_model`` for every target (reference periodogram.py:1229-1269): a
        ``DeviceLightCurveBatch`` with the times of the searched batch and the box model as flux (the weighted mean flux
        inside / outside the transits), resident.  Arguments as in ``compute_stats``."""
        r = self._stats(period, duration, transit_time, True)
        src = self._batch
        out = src._new(src.d_time, r["d_model"], None, src.n_off, nan_free=True, is_sorted=True)
        for m in out.meta:
            m["LABEL"] = "Transit Model Flux"
        return out

    def _fold_box(self, period, transit_time):
        if period is None or transit_time is None:
            pk = self.peaks()
            period = pk["period"] if period is None else period
            transit_time = pk["transit_time"] if transit_time is None else transit_time
        return period, transit_time

    def fold(self, period=None, transit_time=None, **fold_kwargs):
        """The searched batch folded on each target's box: ``self._batch.fold(period, epoch_time=transit_time, ...)`` ->
        ``DeviceFoldedBatch``.  ``period`` / ``transit_time`` (absolute): a scalar or one value per target; None = the value
        at the target's maximum power (``peaks()``).  The transit sits at phase 0."""
        period, transit_time = self._fold_box(period, transit_time)
        return self._batch.fold(period, epoch_time=transit_time, **fold_kwargs)

    def fold_bin(self, period=None, transit_time=None, **kwargs):
        """The same through the fused ``DeviceLightCurveBatch.fold_bin`` (its fold and bin arguments as keywords) ->
        ``DevicePhaseCurveBatch``."""
        period, transit_time = self._fold_box(period, transit_time)
        return self._batch.fold_bin(period, epoch_time=transit_time, **kwargs)

    def river(self, period=None, transit_time=None, **kwargs):
        """The river diagrams of the searched batch on each target's box: ``self._batch.river(period, epoch_time=transit_time,
        ...)`` -> ``DeviceRiverBatch`` (the other keywords are ``DeviceLightCurveBatch.river``'s).  The transit sits at phase 0
        of every row."""
        period, transit_time = self._fold_box(period, transit_time)
        return self._batch.river(period, epoch_time=transit_time, **kwargs)

    def transit_mask(self, period=None, duration=None, transit_time=None, to_host=True):
        """``BoxLeastSquaresPeriodogram.get_transit_mask`` for every target: ``create_transit_mask`` of the searched batch
        with one planet per target (arguments as in ``compute_stats``) -> bool array over its cadences, or the ``DeviceBuffer``
        of bytes (usable as ``flatten(mask=...)``) with ``to_host=False``."""
        period, duration, transit_time = self._box(period, duration, transit_time)
        return self._batch.create_transit_mask(period, transit_time, duration, planet_off=np.arange(self.B + 1, dtype=np.int32),
                                               to_host=to_host)

    def difference_images(self, cubes, period=None, duration=None, transit_time=None, **kwargs):
        """Is each detection on its target's pixels?  ``cubes.difference_images`` (a ``DevicePixelCubeBatch`` holding the
        cutout of every searched target, in the batch's order) at one box per target (arguments as in ``compute_stats``: None =
        the value at the target's maximum power); the other keywords are ``DevicePixelCubeBatch.difference_images``'s."""
        if len(cubes) != self.B:
            raise ValueError("difference_images needs one cutout per searched light curve (%d), got %d" % (self.B, len(cubes)))
        period, duration, transit_time = self._box(period, duration, transit_time)
        return cubes.difference_images(period, transit_time, duration, **kwargs)


# ------------------------------------------------------------------------------------------------ pixel cubes
class DevicePeriodogramBatch(object):
    """B power spectra on ONE frequency grid, in HBM: ``frequency`` (host float64[M], in ``frequency_unit``) and ``power``
    (``DeviceBuffer``, row-major B x M) — what ``DeviceLightCurveBatch.to_periodogram`` returns and the seismology chain of
    the reference consumes one object at a time:

        pg = lc.to_periodogram(normalization="psd"); snr = pg.flatten()          # periodogram.py:381-429
        seis = snr.to_seismology(); seis.estimate_numax(); seis.estimate_deltanu()   # seismology/*_estimators.py

        pgs = batch.to_periodogram(f, normalization="psd")
        res = pgs.estimate_seismology()               # numax, deltanu, status per target; 8 + 16 B per target cross PCIe

    Every method enqueues on the batch's stream; nothing of the size of a spectrum leaves the device unless asked for."""

    def __init__(self, frequency, d_power, B, frequency_unit="uHz", power_unit="", device=0, stream=0):
        self.handle = _capi.Handle.get(device)
        self.device, self.stream = int(device), int(stream or 0)
        self.frequency = np.ascontiguousarray(frequency, dtype=np.float64)
        _pg._freq_unit_factor(frequency_unit)
        if self.frequency.ndim != 1 or self.frequency.size <= 1:
            raise ValueError("frequency and power must have a length greater than 1.")
        self.frequency_unit, self.power_unit = frequency_unit, power_unit
        self.B, self.M = int(B), int(self.frequency.size)
        if d_power.capacity < self.B * self.M * 8:
            raise ValueError("device buffer smaller than the batch it is said to hold")
        self.power = d_power
        self.numax = None                # float64[B] of the last estimate_numax
        self._keep = []                  # host staging the stream may still be reading

    @classmethod
    def from_arrays(cls, frequency, power, frequency_unit="uHz", device=0, stream=0):
        """H2D once: ``frequency`` float64[M] shared by the batch, ``power`` float64[B, M] (one row: [M])."""
        power = np.ascontiguousarray(np.atleast_2d(power), dtype=np.float64)
        frequency = np.asarray(frequency, dtype=np.float64)
        if power.ndim != 2 or frequency.ndim != 1 or power.shape[1] != frequency.size:
            raise ValueError("frequency and power must have the same length.")
        h = _capi.Handle.get(device)
        d_pow, keep = _upload(h, power, stream)
        out = cls(frequency, d_pow, power.shape[0], frequency_unit=frequency_unit, device=device, stream=stream)
        out._keep = [keep]
        return out

    def __len__(self):
        return self.B

    def synchronize(self):
        _capi._check(_capi._lib.lk_stream_synchronize(self.handle._h, _vp(self.stream or None)))
        self._keep = []

    def _is_evenly_spaced(self):
        freqdiff = np.diff(self.frequency)
        return bool(np.allclose(freqdiff[0], freqdiff))

    def _like(self, d_power, power_unit=None):
        out = DevicePeriodogramBatch(self.frequency, d_power, self.B, frequency_unit=self.frequency_unit,
                                     power_unit=self.power_unit if power_unit is None else power_unit, device=self.device,
                                     stream=self.stream)
        out._keep = list(self._keep)
        return out

    def to_host(self):
        """float64[B, M]."""
        out = self.power.download(np.float64, self.B * self.M, stream=self.stream).reshape(self.B, self.M)
        self._keep = []
        return out

    def to_periodograms(self):
        """One host ``Periodogram`` per target."""
        return [_pg.Periodogram(self.frequency, row, frequency_unit=self.frequency_unit, power_unit=self.power_unit)
                for row in self.to_host()]

    def peaks(self):
        """``Periodogram.max_power`` / ``frequency_at_max_power`` (reference periodogram.py:127-140) per target: dict of
        ``max_power``, ``argmax`` (-1 for an all-NaN row) and ``frequency``; 16 B per target cross PCIe."""
        h, B, st = self.handle, self.B, _vp(self.stream or None)
        d_max, d_arg = DeviceBuffer(h, max(B, 1) * 8), DeviceBuffer(h, max(B, 1) * 8)
        if B:
            _capi._check(_capi._lib.lk_argmax_batch_dev(h._h, B, self.M, _vp(self.power.ptr), _vp(d_max.ptr), _vp(d_arg.ptr), st))
        mx = d_max.download(np.float64, B, stream=self.stream)
        am = d_arg.download(np.int64, B, stream=self.stream)
        return dict(max_power=mx, argmax=am, frequency=np.where(am >= 0, self.frequency[np.clip(am, 0, self.M - 1)], np.nan))

    def amplitude_images(self, cubes, **kwargs):
        """Is each spectrum's strongest signal on its target's pixels?  ``cubes.amplitude_images`` (a ``DevicePixelCubeBatch``
        holding the cutout of every target, in the batch's order) at every target's ``peaks()["frequency"]``, in this batch's
        frequency unit; the other keywords are ``DevicePixelCubeBatch.amplitude_images``'s."""
        if len(cubes) != self.B:
            raise ValueError("amplitude_images needs one cutout per spectrum (%d), got %d" % (self.B, len(cubes)))
        return cubes.amplitude_images(self.peaks()["frequency"], freq_unit=self.frequency_unit, **kwargs)

    # ---------------------------------------------------------------- Periodogram.smooth / flatten
    def smooth(self, method="boxkernel", filter_width=0.1):
        """``Periodogram.smooth`` (reference periodogram.py:182-284) of every spectrum -> a new batch; the same planning,
        checks and kernels as the host class (``lk_pg_boxsmooth_batch_dev`` / ``lk_pg_logmedian_batch_dev``)."""
        method = _pg.validate_method(method, ["boxkernel", "logmedian"])
        h, B, M, st, lib = self.handle, self.B, self.M, _vp(self.stream or None), _capi._lib
        if method == "boxkernel":
            if filter_width <= 0.0:
                raise ValueError("the `filter_width` parameter must be larger than 0 for the 'boxkernel' method.")
            if not self._is_evenly_spaced():
                raise ValueError("the 'boxkernel' method requires the periodogram to have a grid of evenly spaced "
                                 "frequencies.")
            fs = np.mean(np.diff(self.frequency))
            taps = np.ascontiguousarray(_pg._box1d_kernel(math.ceil(filter_width / fs))[::-1])
            d_out = DeviceBuffer(h, max(B * M, 1) * 8)
            _capi._check(lib.lk_pg_boxsmooth_batch_dev(h._h, B, M, _vp(self.power.ptr), taps.ctypes.data_as(_dp), int(taps.size),
                                                       _vp(d_out.ptr), st))
            return self._like(d_out)
        tabs = [np.ascontiguousarray(a, dtype=np.int32) for a in _pg._logmedian_windows(self.frequency, filter_width)]
        d_out = DeviceBuffer(h, max(B * M, 1) * 8)
        _capi._check(lib.lk_pg_logmedian_batch_dev(h._h, B, M, _vp(self.power.ptr), int(tabs[0].size), tabs[0].ctypes.data_as(_i32p),
                                                   tabs[1].ctypes.data_as(_i32p), tabs[2].ctypes.data_as(_i32p),
                                                   tabs[3].ctypes.data_as(_i32p), (8.0 / 9.0) ** 3, _vp(d_out.ptr), st))
        return self._like(d_out)

    def flatten(self, method="logmedian", filter_width=0.01, return_trend=False):
        """``Periodogram.flatten`` (reference periodogram.py:381-429): power / smooth, unitless, as a new batch (and the
        background batch with ``return_trend``); the division is ``lk_pg_snr_batch_dev``."""
        bkg = self.smooth(method=method, filter_width=filter_width)
        d_snr = DeviceBuffer(self.handle, max(self.B * self.M, 1) * 8)
        _capi._check(_capi._lib.lk_pg_snr_batch_dev(self.handle._h, self.B, self.M, _vp(self.power.ptr), _vp(bkg.power.ptr),
                                                    _vp(d_snr.ptr), _vp(self.stream or None)))
        snr = self._like(d_snr, power_unit="")
        return (snr, bkg) if return_trend else snr

    # ---------------------------------------------------------------- seismology
    def estimate_numax(self, numaxs=None, window_width=None, spacing=None, return_metric=False):
        """``estimate_numax_acf2d`` (reference seismology/numax_estimators.py:15-205) per target, resident: the plan and its
        ``ValueError``s are ``seismology._plan``'s on the shared grid; ``lk_pg_acf_metric_batch_dev`` forms the metric of
        every window without storing the 2-D ACF, ``lk_pg_numax_pick_batch_dev`` smooths it and takes the argmax; 8 B per
        target come back.  Returns a dict: ``numax`` float64[B] (also kept as ``self.numax``), ``numaxs``, ``window_width``
        and, with ``return_metric``, ``metric`` and ``metric_smooth`` (float64[B, len(numaxs)])."""
        numaxs, window_width, starts, W = _seis._plan(self, numaxs, window_width, spacing)
        h, B, M, st, lib = self.handle, self.B, self.M, _vp(self.stream or None), _capi._lib
        n_win = int(numaxs.size)
        if n_win == 0:
            raise ValueError("attempt to get argmax of an empty sequence")
        if starts.min() < 0 or int(starts.max()) + W > M:
            raise ValueError("a window reaches outside the spectrum")
        ws = np.ascontiguousarray(starts, dtype=np.int32)
        d_met, d_smooth = DeviceBuffer(h, max(B * n_win, 1) * 8), DeviceBuffer(h, max(B * n_win, 1) * 8)
        d_arg = DeviceBuffer(h, max(B, 1) * 8)
        taps = np.ascontiguousarray(_seis._gaussian_taps(np.sqrt(n_win))) if n_win > 10 else None
        _capi._check(lib.lk_pg_acf_metric_batch_dev(h._h, B, M, _vp(self.power.ptr), n_win, ws.ctypes.data_as(_i32p), W,
                                                    _vp(d_met.ptr), st))
        _capi._check(lib.lk_pg_numax_pick_batch_dev(h._h, B, n_win, _vp(d_met.ptr), None if taps is None else taps.ctypes.data_as(_dp),
                                                    0 if taps is None else int(taps.size), _vp(d_smooth.ptr), _vp(d_arg.ptr), st))
        arg = d_arg.download(np.int64, B, stream=self.stream)
        self.numax = numaxs[arg]
        out = dict(numax=self.numax, numaxs=numaxs, window_width=window_width)
        if return_metric:
            out["metric"] = d_met.download(np.float64, B * n_win, stream=self.stream).reshape(B, n_win)
            out["metric_smooth"] = d_smooth.download(np.float64, B * n_win, stream=self.stream).reshape(B, n_win)
        return out

    def estimate_deltanu(self, numax=None, return_acf=False):
        """``estimate_deltanu_acf2d`` (reference seismology/deltanu_estimators.py:18-153) per target, each around its own
        ``numax``: a scalar, one value per target, or None for the last ``estimate_numax`` result.  The windows are planned
        on the host from those B numbers (``seismology._deltanu_plan``), ``lk_pg_deltanu_batch_dev`` does the rest.  Returns a
        dict of arrays [B]: ``deltanu`` (NaN unless ``status`` is 0), ``deltanu_emp``, ``n_peaks``, ``status`` (0 ok, 1 skipped:
        numax NaN or <= 0, 2 no usable window, 3 no peak in the selection; no target raises) and ``numax``; with
        ``return_acf`` also ``acf`` float64[B, max_sel] (the rescaled ACF on the selected lags, NaN behind them), ``sel_lo``
        and ``sel_len``."""
        if numax is None:
            if self.numax is None:
                raise ValueError("pass numax or call estimate_numax first")
            numax = self.numax
        if not self._is_evenly_spaced():
            raise ValueError("the ACF 2D method requires that the periodogram has a grid of uniformly spaced frequencies.")
        h, B, M, st = self.handle, self.B, self.M, _vp(self.stream or None)
        numax = np.ascontiguousarray(np.broadcast_to(np.asarray(numax, dtype=np.float64), (B,)))
        plan = _seis._deltanu_plan(self.frequency, self.frequency_unit, numax)
        tabs, max_sel = _capi._deltanu_tables(plan, B)
        d_dnu = DeviceBuffer(h, max(B, 1) * 8)
        d_int = DeviceBuffer(h, max(B, 1) * 16)                     # n_peaks | status | sel_lo | sel_len, int32[B] each
        d_acf = DeviceBuffer(h, max(B * max_sel, 1) * 8) if return_acf else None
        _capi._check(_capi._lib.lk_pg_deltanu_batch_dev(
            h._h, B, M, _vp(self.power.ptr), tabs[0].ctypes.data_as(_i32p), tabs[1].ctypes.data_as(_i32p), tabs[2].ctypes.data_as(_dp),
            tabs[3].ctypes.data_as(_dp), tabs[4].ctypes.data_as(_dp), tabs[5].ctypes.data_as(_dp), max_sel, _vp(d_dnu.ptr),
            _vp(d_int.ptr), _vp(d_int.ptr + 4 * B), _vp(d_int.ptr + 8 * B), _vp(d_int.ptr + 12 * B),
            _vp(d_acf.ptr if d_acf is not None else None), st))
        ints = d_int.download(np.int32, 4 * B, stream=self.stream).reshape(4, B)
        out = dict(deltanu=d_dnu.download(np.float64, B, stream=self.stream), deltanu_emp=plan["deltanu_emp"], n_peaks=ints[0],
                   status=ints[1], numax=numax)
        if return_acf:
            out.update(acf=d_acf.download(np.float64, B * max_sel, stream=self.stream).reshape(B, max_sel), sel_lo=ints[2],
                       sel_len=ints[3])
        return out

    def estimate_seismology(self, method="logmedian", filter_width=0.01, numaxs=None, window_width=None, spacing=None):
        """The reference's chain ``pg.flatten().to_seismology()``, ``estimate_numax()``, ``estimate_deltanu()`` for the batch:
        dict of ``numax``, ``deltanu``, ``deltanu_emp``, ``n_peaks`` and ``status`` (of the deltanu step) per target."""
        snr = self.flatten(method=method, filter_width=filter_width)
        numax = snr.estimate_numax(numaxs=numaxs, window_width=window_width, spacing=spacing)["numax"]
        self.numax = numax
        res = snr.estimate_deltanu(numax)
        return dict(numax=numax, deltanu=res["deltanu"], deltanu_emp=res["deltanu_emp"], n_peaks=res["n_peaks"], status=res["status"])


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
                h._h, _vp(d_raw.ptr), int(row_bytes), int(n_rows), int(pc["off_time"]), int(pc["code_time"]),
                int(pc["off_quality"]), int(pc["code_quality"]), ctypes.c_int64(int(pc["bitmask"])), int(bool(pc["keep_nan_time"])),
                2, cols.ctypes.data_as(_i32p), npix, _vp(d_t.ptr), _vp(d_q.ptr), _vp(d_c.ptr), _off_ptr(kept), st))
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

    def to_host(self):
        """D2H of the cubes -> list of ``PixelCube`` (round trip, for tests)."""
        from .correctors.pldcorrector import PixelCube
        B, N, ny, nx = self.shape
        f = self.d_flux.download(np.float32, B * N * ny * nx, stream=self.stream).reshape(self.shape)
        e = self.d_flux_err.download(np.float32, B * N * ny * nx, stream=self.stream).reshape(self.shape)
        t = self.d_time.download(np.float64, B * N, stream=self.stream).reshape(B, N)
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
        _capi._check(_capi._lib.lk_cube_median_image_batch_dev(self.handle._h, B, N, ny * nx, _vp(self.d_flux.ptr),
                                                               _vp(d_keep.ptr if d_keep is not None else None), _vp(d_med.ptr),
                                                               _vp(self.stream or None)))
        return d_med

    def median_images(self, d_keep=None):
        """np.nanmedian(flux.astype(float64), axis=0) of every cutout, computed on the device (``lk_cube_median_image_batch_dev``)
        over all cadences or those flagged in ``d_keep`` (DeviceBuffer of B x N bytes) -> float64[B, ny, nx] on the host."""
        B, N, ny, nx = self.shape
        return self._median_images_dev(d_keep).download(np.float64, B * ny * nx, stream=self.stream).reshape(B, ny, nx)

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
            h._h, B, ny, nx, _vp(d_med.ptr), float(threshold), int(use_ref), float(reference_pixel[0]) if use_ref else 0.0,
            float(reference_pixel[1]) if use_ref else 0.0, int(bool(invert)), _vp(d_mask.ptr), _vp(d_cnt.ptr), _vp(d_idx.ptr),
            _vp(self.stream or None)))
        if not to_host:
            return d_mask, d_cnt, d_idx         # (d_med goes back to the pool: its next user is ordered behind this stream's kernel)
        return d_mask.download(np.uint8, B * npix, stream=self.stream).reshape(B, ny, nx).astype(bool)

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

    def _aperture(self, aperture_mask):
        """``lk_cube_aperture_batch_dev``: -> (d_flux32, d_err32, d_keep, kept[B], nonfinite[B])."""
        h, (B, N, ny, nx) = self.handle, self.shape
        ap = self._masks(aperture_mask, True, None, {})
        d_mask, k = _upload(h, ap.reshape(-1, ny * nx), self.stream, np.uint8)
        d_f, d_e, d_k = DeviceBuffer(h, B * N * 4), DeviceBuffer(h, B * N * 4), DeviceBuffer(h, B * N)
        kept, dirty = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        _capi._check(_capi._lib.lk_cube_aperture_batch_dev(h._h, B, N, ny * nx, _vp(self.d_flux.ptr), _vp(self.d_flux_err.ptr),
                                                           _vp(d_mask.ptr), ny * nx if ap.ndim == 3 else 0, _vp(d_f.ptr),
                                                           _vp(d_e.ptr), _vp(d_k.ptr), _off_ptr(kept), _off_ptr(dirty),
                                                           _vp(self.stream or None)))           # (synchronises)
        del k
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

        def ptr(key):
            return _vp(out[key].ptr if out[key] is not None else None)

        def idx(a):
            return (None, 0) if a is None else (a.ctypes.data_as(_i32p), a.shape[1] if a.shape[0] > 1 else 0)

        def didx(a):
            return (None, 0) if a is None else (_vp(a[0].ptr), int(a[1]))

        (pi, ps), (bi, bs) = (didx(pld_idx), didx(bkg_idx)) if ragged else (idx(pld_idx), idx(bkg_idx))
        flag = np.zeros(1, dtype=np.int32)
        fn = _capi._lib.lk_pld_gather_ragged_batch_dev if ragged else _capi._lib.lk_pld_gather_batch_dev
        _capi._check(fn(
            h._h, B, N, ny * nx, n, _vp(self.d_flux.ptr), _vp(self.d_time.ptr), _vp(d_f.ptr), _vp(d_e.ptr), _vp(d_k.ptr), int(P), pi,
            ps, int(Pb), bi, bs, n_inner, None if lo is None or not n_inner else lo.ctypes.data_as(_i32p),
            None if g is None or not n_inner else g.ctypes.data_as(_dp), ptr("time"), ptr("y"), ptr("err"), ptr("lcf"), ptr("pld"),
            ptr("bkg"), ptr("knots"), flag.ctypes.data_as(_i32p), _vp(self.stream or None)))      # (synchronises)
        out["nonfinite"] = bool(flag[0])
        return out

    # ---------------------------------------------------------------- aperture photometry
    def to_lightcurves(self, aperture_mask="all"):
        """``PixelCube.to_lightcurve(aperture_mask)`` of every cutout without its NaN cadences (what ``PLDCorrector.__init__``
        keeps, pldcorrector.py:109-120), resident -> ``DeviceLightCurveBatch`` (float64 = the float32 sums widened)."""
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
        ap = self._masks(aperture_mask, True, None, {})
        d_mask, k = _upload(h, ap.reshape(-1, ny * nx), self.stream, np.uint8)
        d_c, d_r = DeviceBuffer(h, B * N * 8), DeviceBuffer(h, B * N * 8)
        d_p = DeviceBuffer(h, B * N * 4) if return_peak else None
        args = (h._h, B, N, ny * nx, nx, _vp(self.d_flux.ptr), _vp(d_mask.ptr), ny * nx if ap.ndim == 3 else 0, float(column),
                float(row), _vp(d_c.ptr), _vp(d_r.ptr))
        if method == "quadratic":
            _capi._check(_capi._lib.lk_cube_centroids_quadratic_batch_dev(*args, _vp(d_p.ptr if return_peak else None),
                                                                          _vp(self.stream or None)))
        else:
            _capi._check(_capi._lib.lk_cube_centroids_batch_dev(*args, _vp(self.stream or None)))
        self._keep.append(k)
        if not to_host:
            return (d_c, d_r, d_p) if return_peak else (d_c, d_r)
        out = (d_c.download(np.float64, B * N, stream=self.stream).reshape(B, N),
               d_r.download(np.float64, B * N, stream=self.stream).reshape(B, N))
        return out + (d_p.download(np.int32, B * N, stream=self.stream).reshape(B, N),) if return_peak else out

    # ---------------------------------------------------------------- background
    def _background(self, aperture_mask, want_scatter, subtract):
        """One launch of ``lk_cube_background_batch_dev`` -> (masks bool (B, ny, nx), d_bkg, d_n_pixels, d_scatter or None,
        d_cube_out or None), enqueued on the batch's stream."""
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
        m = self._masks(aperture_mask, False, None, {})
        d_mask, k = _upload(h, m.reshape(-1, npix), self.stream, np.uint8)
        d_bkg, d_n = DeviceBuffer(h, B * N * 4), DeviceBuffer(h, B * N * 4)
        d_sc = DeviceBuffer(h, B * N * 4) if want_scatter else None
        d_out = DeviceBuffer(h, B * N * npix * 4) if subtract else None
        _capi._check(_capi._lib.lk_cube_background_batch_dev(
            h._h, B, N, npix, _vp(self.d_flux.ptr), _vp(d_mask.ptr), npix if m.ndim == 3 else 0, int(bool(want_scatter)),
            _vp(d_bkg.ptr), _vp(d_n.ptr), _vp(d_sc.ptr if want_scatter else None), _vp(d_out.ptr if subtract else None),
            _vp(self.stream or None)))
        self._keep.extend([k, d_mask])
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
                    out[key] = out[key].download(dt, B * N, stream=self.stream).reshape(B, N)
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
            bkg = d_bkg.download(np.float32, B * N, stream=self.stream).reshape(B, N)
            info = {"flux": bkg, "mask": m}
            if return_background:
                info["n_pixels"] = d_n.download(np.int32, B * N, stream=self.stream).reshape(B, N)
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
                bkg = d_rows.download(np.float32, B * N, stream=self.stream).reshape(B, N)
            else:
                bkg = np.asarray(background, dtype=np.float32)
                if bkg.shape != (B, N):
                    raise ValueError("background must be (B, N) = %r, one value per cadence (got %r)" % ((B, N), bkg.shape))
                d_rows, keep = _upload(h, bkg, self.stream, np.float32)
            if isinstance(info.get("n_pixels"), DeviceBuffer):
                info["n_pixels"] = info["n_pixels"].download(np.int32, B * N, stream=self.stream).reshape(B, N)
            info["flux"] = bkg
            d_out = DeviceBuffer(h, B * N * npix * 4)
            _capi._check(_capi._lib.lk_cube_subtract_rows_batch_dev(h._h, B, N, npix, _vp(self.d_flux.ptr), _vp(d_rows.ptr),
                                                                    _vp(d_out.ptr), _vp(self.stream or None)))
        nan_cadences = np.isnan(bkg).sum(axis=1)
        meta = [dict(mb, BKG_SUBTRACTED=True, BKG_NPIX=int(counts[b]), BKG_NAN_CADENCES=int(nan_cadences[b]))
                for b, mb in enumerate(self.meta)]          # (the keys of PixelCube.subtract_background)
        out = DevicePixelCubeBatch(self.d_time, d_out, self.d_flux_err, self.time, self.shape, meta, self.device, self.stream,
                                   is_sorted=self.is_sorted)
        if background is not None:
            out._keep = [keep, d_rows]          # what the enqueued subtraction still reads
        return (out, info) if return_background else out

    # ---------------------------------------------------------------- difference images
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
        box = []
        for name, a in (("period", period), ("transit_time", transit_time), ("duration", duration)):
            a = np.asarray(a, dtype=np.float64)
            if a.ndim > 1 or (a.ndim == 1 and a.size != B):
                raise ValueError("%s must be a scalar or one value per cutout (%d), got shape %r" % (name, B, a.shape))
            if not np.all(np.isfinite(a)):
                raise ValueError("%s must be finite" % name)
            box.append(np.ascontiguousarray(np.broadcast_to(a, (B,))))
        if np.any(box[0] == 0):
            raise ValueError("period must be non-zero")
        if ny < 3 or nx < 3:
            raise ValueError("the quadratic centroid needs cutouts of at least 3 x 3 pixels (got %d x %d)" % (ny, nx))
        ap = self._masks(aperture_mask, True, None, {})
        d_mask, k = _upload(h, ap.reshape(-1, npix), self.stream, np.uint8)
        mask_stride = npix if ap.ndim == 3 else 0
        st = _vp(self.stream or None)
        img = {key: DeviceBuffer(h, B * npix * 8) for key in ("mean_in", "mean_out", "diff", "diff_err")}
        d_cls, d_nin, d_nout = DeviceBuffer(h, B * N), DeviceBuffer(h, B * 4), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_cube_diffimage_batch_dev(
            h._h, B, N, npix, _vp(self.d_time.ptr), _vp(self.d_flux.ptr), _vp(self.d_flux_err.ptr), box[0].ctypes.data_as(_dp),
            box[1].ctypes.data_as(_dp), box[2].ctypes.data_as(_dp), float(in_width), float(out_inner), float(out_outer),
            _vp(d_cls.ptr), _vp(img["mean_in"].ptr), _vp(img["mean_out"].ptr), _vp(img["diff"].ptr), _vp(img["diff_err"].ptr),
            _vp(d_nin.ptr), _vp(d_nout.ptr), st))
        cen = {}
        for key, src, method in (("centroid_diff", "diff", 1), ("centroid_out", "mean_out", 1),
                                 ("centroid_diff_moments", "diff", 0), ("centroid_out_moments", "mean_out", 0)):
            cen[key] = (DeviceBuffer(h, B * 8), DeviceBuffer(h, B * 8))
            _capi._check(_capi._lib.lk_image_centroids_batch_dev(
                h._h, B, npix, nx, _vp(img[src].ptr), _vp(d_mask.ptr), mask_stride, float(column), float(row), method,
                _vp(cen[key][0].ptr), _vp(cen[key][1].ptr), _vp(None), st))
        d_off, d_pix, d_status = DeviceBuffer(h, B * 16), DeviceBuffer(h, B * 8), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_diffimage_offsets_batch_dev(
            h._h, B, _vp(d_nin.ptr), _vp(d_nout.ptr), _vp(cen["centroid_diff"][0].ptr), _vp(cen["centroid_diff"][1].ptr),
            _vp(cen["centroid_out"][0].ptr), _vp(cen["centroid_out"][1].ptr), _vp(d_off.ptr), _vp(d_pix.ptr), _vp(d_status.ptr), st))
        out = dict(n_in=d_nin.download(np.int32, B, stream=self.stream), n_out=d_nout.download(np.int32, B, stream=self.stream),
                   status=d_status.download(np.int32, B, stream=self.stream))       # (synchronises: the staged mask may go)
        del k
        if not to_host:
            out.update(img, offset=d_off, offset_pix=d_pix, cadence_class=d_cls, **cen)
            return out
        for key, buf in img.items():
            out[key] = buf.download(np.float64, B * npix, stream=self.stream).reshape(B, ny, nx)
        for key, (d_c, d_r) in cen.items():
            out[key] = np.stack([d_c.download(np.float64, B, stream=self.stream), d_r.download(np.float64, B, stream=self.stream)],
                                axis=1)
        out["offset"] = d_off.download(np.float64, 2 * B, stream=self.stream).reshape(B, 2)
        out["offset_pix"] = d_pix.download(np.float64, B, stream=self.stream)
        out["cadence_class"] = d_cls.download(np.uint8, B * N, stream=self.stream).reshape(B, N)
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
        if freq.ndim > 1 or (freq.ndim == 1 and freq.size != B):
            raise ValueError("frequency must be a scalar or one value per cutout (%d), got shape %r" % (B, freq.shape))
        f_day = np.ascontiguousarray(np.broadcast_to(freq, (B,)) / _freq_unit_factor(freq_unit if freq_unit is not None else "1/d"))
        if ny < 3 or nx < 3:
            raise ValueError("the quadratic centroid needs cutouts of at least 3 x 3 pixels (got %d x %d)" % (ny, nx))
        fin = np.isfinite(self.time)
        first = np.argmax(fin, axis=1)
        t_ref = np.ascontiguousarray(np.where(fin.any(axis=1), self.time[np.arange(B), first], np.nan))
        ap = self._masks(aperture_mask, True, None, {})
        d_mask, k = _upload(h, ap.reshape(-1, npix), self.stream, np.uint8)
        mask_stride = npix if ap.ndim == 3 else 0
        st = _vp(self.stream or None)
        img = {key: DeviceBuffer(h, n * B * npix * 8) for key, n in (("theta", K), ("level", 1), ("amplitude", nterms), ("phase", nterms),
                                                                   ("amplitude_err", nterms), ("snr", nterms), ("chi2", 1))}
        d_used, d_fit = DeviceBuffer(h, B * npix * 4), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_cube_ampimage_batch_dev(
            h._h, B, N, npix, _vp(self.d_time.ptr), _vp(self.d_flux.ptr), f_day.ctypes.data_as(_dp), nterms, t_ref.ctypes.data_as(_dp),
            _vp(img["theta"].ptr), _vp(img["level"].ptr), _vp(img["amplitude"].ptr), _vp(img["phase"].ptr),
            _vp(img["amplitude_err"].ptr), _vp(img["snr"].ptr), _vp(img["chi2"].ptr), _vp(d_used.ptr), _vp(d_fit.ptr), st))
        cen = {}
        for key, src, method in (("centroid_amp", "amplitude", 1), ("centroid_level", "level", 1),
                                 ("centroid_amp_moments", "amplitude", 0), ("centroid_level_moments", "level", 0)):
            cen[key] = (DeviceBuffer(h, B * 8), DeviceBuffer(h, B * 8))       # (amplitude's first block is harmonic 1 of the batch)
            _capi._check(_capi._lib.lk_image_centroids_batch_dev(
                h._h, B, npix, nx, _vp(img[src].ptr), _vp(d_mask.ptr), mask_stride, float(column), float(row), method,
                _vp(cen[key][0].ptr), _vp(cen[key][1].ptr), _vp(None), st))
        d_off, d_pix, d_status = DeviceBuffer(h, B * 16), DeviceBuffer(h, B * 8), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_ampimage_offsets_batch_dev(
            h._h, B, _vp(d_fit.ptr), _vp(cen["centroid_amp"][0].ptr), _vp(cen["centroid_amp"][1].ptr),
            _vp(cen["centroid_level"][0].ptr), _vp(cen["centroid_level"][1].ptr), _vp(d_off.ptr), _vp(d_pix.ptr), _vp(d_status.ptr), st))
        out = dict(status=d_status.download(np.int32, B, stream=self.stream), frequency=f_day, t_ref=t_ref)   # (synchronises)
        del k
        if not to_host:
            out.update(img, n_used=d_used, offset=d_off, offset_pix=d_pix, **cen)
            return out
        for key, n in (("theta", K), ("amplitude", nterms), ("phase", nterms), ("amplitude_err", nterms), ("snr", nterms)):
            a = img[key].download(np.float64, n * B * npix, stream=self.stream).reshape(n, B, ny, nx)
            out[key] = np.ascontiguousarray(a.transpose(1, 0, 2, 3))
        for key in ("level", "chi2"):
            out[key] = img[key].download(np.float64, B * npix, stream=self.stream).reshape(B, ny, nx)
        out["n_used"] = d_used.download(np.int32, B * npix, stream=self.stream).reshape(B, ny, nx)
        for key, (d_c, d_r) in cen.items():
            out[key] = np.stack([d_c.download(np.float64, B, stream=self.stream), d_r.download(np.float64, B, stream=self.stream)],
                                axis=1)
        out["offset"] = d_off.download(np.float64, 2 * B, stream=self.stream).reshape(B, 2)
        out["offset_pix"] = d_pix.download(np.float64, B, stream=self.stream)
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
        fin = np.isfinite(self.time)
        first = np.argmax(fin, axis=1)
        t_ref = np.ascontiguousarray(np.where(fin.any(axis=1), self.time[np.arange(B), first], np.nan))
        st = _vp(self.stream or None)
        d_power = DeviceBuffer(h, power_bytes) if return_power else None
        d_peak, d_idx = DeviceBuffer(h, B * npix * 8), DeviceBuffer(h, B * npix * 4)
        d_used, d_status = DeviceBuffer(h, B * npix * 4), DeviceBuffer(h, B * 4)
        _capi._check(_capi._lib.lk_cube_pixel_ls_batch_dev(
            h._h, B, N, npix, _vp(self.d_time.ptr), _vp(self.d_flux.ptr), f_day.ctypes.data_as(_dp), F, norms[normalization], osf,
            t_ref.ctypes.data_as(_dp), _vp(d_power.ptr if return_power else None), _vp(d_peak.ptr), _vp(d_idx.ptr), _vp(d_used.ptr),
            _vp(d_status.ptr), st))
        out = dict(status=d_status.download(np.int32, B, stream=self.stream), t_ref=t_ref, frequency=f_day)    # (synchronises)
        if not to_host:
            out.update(peak_power=d_peak, peak_index=d_idx, n_used=d_used)
            if return_power:
                out["power"] = d_power
            return out
        if return_power:
            out["power"] = d_power.download(np.float64, B * F * npix, stream=self.stream).reshape(B, F, ny, nx)
        out["peak_power"] = d_peak.download(np.float64, B * npix, stream=self.stream).reshape(B, ny, nx)
        out["peak_index"] = d_idx.download(np.int32, B * npix, stream=self.stream).reshape(B, ny, nx)
        out["peak_frequency"] = np.where(out["peak_index"] >= 0, f_day[np.clip(out["peak_index"], 0, F - 1)], np.nan)
        out["n_used"] = d_used.download(np.int32, B * npix, stream=self.stream).reshape(B, ny, nx)
        return out

    # ---------------------------------------------------------------- PSF photometry
    def psf_photometry(self, star_col, star_row, sigma, shifts=None, aperture_mask="all", column=0, row=0, use_flux_err=True,
                       to_host=False):
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
        batch position and from run to run."""
        from .correctors.pldcorrector import _psf_sigma
        h, (B, N, ny, nx) = self.handle, self.shape
        npix = ny * nx
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
        S_max = pos[0].shape[1]
        part = ~(np.isnan(pos[0]) | np.isnan(pos[1]))
        if not np.all(np.isfinite(pos[0][part]) & np.isfinite(pos[1][part])):
            raise ValueError("a star position is infinite")
        if not np.all(part.any(axis=1)):
            raise ValueError("cutouts %s have no star" % np.flatnonzero(~part.any(axis=1)).tolist())
        sg = np.asarray(sigma, dtype=np.float64)
        sg = np.array([_psf_sigma(s) for s in sg]) if sg.shape == (B, 2) else np.tile(_psf_sigma(sg), (B, 1))
        sg = np.ascontiguousarray(sg, dtype=np.float64)
        keep = []
        d_shift = [None, None]
        if shifts is not None:
            if len(shifts) != 2:
                raise ValueError("shifts must be a pair (shift_col, shift_row)")
            for i, a in enumerate(shifts):
                if isinstance(a, DeviceBuffer):
                    if a.nbytes != B * N * 8:
                        raise ValueError("a shift buffer of %d bytes for %d x %d float64 cadences" % (a.nbytes, B, N))
                    d_shift[i] = a
                else:
                    a = np.asarray(a, dtype=np.float64)
                    if a.shape != (B, N):
                        raise ValueError("shifts must be (B, N) = %r arrays (got %r)" % ((B, N), a.shape))
                    d_shift[i], k = _upload(h, a, self.stream, np.float64)
                    keep.append(k)
        m = self._masks(aperture_mask, False, None, {})
        d_mask, k = _upload(h, m.reshape(-1, npix), self.stream, np.uint8)
        keep.append(k)
        rows = int(part.sum())
        d_t, d_f, d_e = (DeviceBuffer(h, rows * N * 8) for _ in range(3))
        d_bkg, d_chi = DeviceBuffer(h, B * N * 8), DeviceBuffer(h, B * N * 8)
        d_n, d_cs, d_st = DeviceBuffer(h, B * N * 4), DeviceBuffer(h, B * N), DeviceBuffer(h, B * 4)
        star_off = np.zeros(B + 1, dtype=np.int32)
        _capi._check(_capi._lib.lk_cube_psf_photometry_batch_dev(
            h._h, B, N, ny, nx, _vp(self.d_time.ptr), _vp(self.d_flux.ptr), _vp(self.d_flux_err.ptr), _vp(d_mask.ptr),
            npix if m.ndim == 3 else 0, S_max, pos[0].ctypes.data_as(_dp), pos[1].ctypes.data_as(_dp), sg.ctypes.data_as(_dp),
            _vp(d_shift[0].ptr if shifts is not None else None), _vp(d_shift[1].ptr if shifts is not None else None),
            float(column), float(row), int(bool(use_flux_err)), star_off.ctypes.data_as(_i32p), _vp(d_t.ptr), _vp(d_f.ptr),
            _vp(d_e.ptr), _vp(d_bkg.ptr), _vp(d_chi.ptr), _vp(d_n.ptr), _vp(d_cs.ptr), _vp(d_st.ptr), _vp(self.stream or None)))
        meta = [dict(self.meta[b], STAR_INDEX=int(s), STAR_COL=float(pos[0][b, s]), STAR_ROW=float(pos[1][b, s]))
                for b in range(B) for s in np.flatnonzero(part[b])]
        lcs = DeviceLightCurveBatch(d_t, d_f, d_e, np.arange(rows + 1, dtype=np.int64) * N, meta, self.device, self.stream,
                                    is_sorted=True if self.is_sorted else None)
        lcs._keep = keep + [d_mask] + [d for d in d_shift if d is not None]       # what the enqueued fit still reads
        info = {"background": d_bkg, "chi2": d_chi, "n_used": d_n, "cadence_status": d_cs, "status": d_st}
        if not to_host:
            info["star_off"], k = _upload(h, star_off, self.stream, np.int32)
            lcs._keep.append(k)
            return lcs, info
        for key, dt, shp in (("background", np.float64, (B, N)), ("chi2", np.float64, (B, N)), ("n_used", np.int32, (B, N)),
                             ("cadence_status", np.int8, (B, N)), ("status", np.int32, (B,))):
            info[key] = info[key].download(dt, int(np.prod(shp)), stream=self.stream).reshape(shp)
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
        args = (h._h, B, n, P, Pb, _vp(d_pld.ptr if d_pld is not None else None), _vp(d_bkg.ptr), _vp(g["lcf"].ptr), _vp(g["time"].ptr),
                _vp(g["knots"].ptr), n_inner, int(pld_order), int(pca_components), n_knots, int(spline_degree),
                int(bool(normalize_background_pixels)), K, _vp(g["y"].ptr), _vp(g["err"].ptr), _vp(d_cm.ptr if d_cm is not None else None),
                float(sigma), int(niters), _vp(d_X.ptr), _vp(d_ps.ptr), _vp(d_mu.ptr), _vp(d_w.ptr), _vp(d_model.ptr), _vp(d_outl.ptr),
                _vp(d_sp.ptr if d_sp is not None else None), _vp(d_corr.ptr), _vp(self.stream or None))
        if ragged:
            _capi._check(_capi._lib.lk_pld_correct_ragged_batch_dev(*args, _vp(d_pc.ptr if d_pc is not None else None),
                                                                    _vp(d_bc.ptr if d_bc is not None else None)))
        else:
            _capi._check(_capi._lib.lk_pld_correct_batch_dev(*args))
        if to_host:
            corrected = d_corr.download(np.float64, B * n, stream=self.stream).reshape(B, n)
            outl = d_outl.download(np.uint8, B * n, stream=self.stream).reshape(B, n).astype(bool)
            return corrected, outl
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
