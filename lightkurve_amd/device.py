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
from .cubes import DevicePixelCubeBatch  # noqa: F401  (cubes.py imports this module only inside its methods)
from .devmem import DeviceBuffer, _Pool, _dp, _i32p, _ip, _off_ptr, _pool, _upload, _vp, release_device_pool  # noqa: F401

__all__ = ["DeviceBuffer", "DeviceLightCurveBatch", "DeviceFoldedBatch", "DevicePhaseCurveBatch", "DeviceBLSResult",
           "DevicePeriodogramBatch", "DevicePixelCubeBatch", "release_device_pool"]



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
