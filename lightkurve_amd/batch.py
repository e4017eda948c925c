"""Batched (many targets at once) entry points of the hot path, sharded over ranks when a process group exists.

These are what a pipeline over a ``LightCurveCollection`` (reference: src/lightkurve/collections.py:145) calls
instead of looping ``lc.to_periodogram()`` / ``lc.flatten()`` per target."""
import numpy as np

from . import _capi
from .distributed import all_gather_rows, device_gather_available, shard_bounds, sharded_map, sharded_map_ragged
from . import packed

__all__ = ["lombscargle_batch", "lombscargle_peaks_batch", "bls_batch", "bls_stats_batch", "ls_model_batch", "fold_bin_batch", "river_batch", "fill_gaps_batch",
           "periodogram_peaks", "flatten_batch",
           "estimate_cdpp_batch", "pld_correct_batch", "difference_images_batch", "amplitude_images_batch", "psf_photometry_batch", "psf_fit_batch", "psf_width_batch", "psf_positions_batch", "pixel_periodograms_batch", "subtract_background_batch", "regression_correct_batch", "cbv_correct_batch"]


def _resolve_device(device):
    """The GPU this process drives: ``device`` if given; otherwise torch's current device under a RCCL process group
    (one process per GPU: the launcher's LOCAL_RANK -> torch.cuda.set_device), else 0."""
    if device is not None:
        return int(device)
    if device_gather_available():
        import torch
        return int(torch.cuda.current_device())
    return 0


def _slice_packed(cols, n_off, b0, b1):
    a, b = int(n_off[b0]), int(n_off[b1])
    return [c[a:b] for c in cols], n_off[b0:b1 + 1] - n_off[b0]


def _local_packed(lcs, columns, prefix="pack", pinned="auto"):
    """This rank's block of the batch as packed arrays -> (columns, n_off, bounds).  ``lcs``: a ``LightCurveBatch`` (its
    arrays are used as they are; a block is a slice) or an iterable of light curves (one concatenation per column into
    the pinned staging pool).  Without a process group the block is the whole batch and ``bounds`` is None; with one the
    batch is cut into contiguous blocks balanced by cadence count (distributed.shard_bounds) BEFORE packing, so a rank
    only touches its own light curves."""
    from .distributed import _dist
    from .ingest import LightCurveBatch
    dist = _dist()
    multi = dist is not None and dist.is_initialized()
    if isinstance(lcs, LightCurveBatch):
        cols, n_off = [getattr(lcs, c) for c in columns], lcs.n_off
        if not multi:
            return cols, n_off, None
        bounds = shard_bounds(len(n_off) - 1, dist.get_world_size(), np.diff(n_off))
        r = dist.get_rank()
        c, o = _slice_packed(cols, n_off, int(bounds[r]), int(bounds[r + 1]))
        return c, o, bounds
    lcs = list(lcs)
    bounds = None
    if multi:
        bounds = shard_bounds(len(lcs), dist.get_world_size(), [len(lc.time) for lc in lcs])
        r = dist.get_rank()
        lcs = lcs[int(bounds[r]):int(bounds[r + 1])]
    cols, n_off = packed.pack_columns(lcs, columns, pinned=pinned, pool_prefix=prefix)
    return cols, n_off, bounds


def _finish(local, bounds, gather):
    return all_gather_rows(local, bounds) if (bounds is not None and gather) else local


def _ls_power_packed(time, flux, n_off, plan, device, want_power=True, want_peaks=False, out=None):
    """Lomb-Scargle of a packed batch on the plan's shared grid -> (power[B, M] or None, max[B] or None, argmax[B] or None).
    One vectorised NaN pass and one endpoint gather on the host; ``ls_method="fast"`` hands the absolute times to
    ``lk_ls_fast_peaks_lc_batch`` (rebased on the device), the exact methods rebase in one numpy pass."""
    time, flux, n_off = packed.drop_nan_flux(time, flux, n_off)
    counts = np.diff(n_off)
    B, M = len(counts), len(plan.f_day)
    if B == 0:
        return (np.zeros((0, M)) if want_power else None, np.zeros(0) if want_peaks else None,
                np.zeros(0, np.int64) if want_peaks else None)
    if counts.min() < 2:
        raise ValueError("The light curve needs at least two cadences to build a periodogram.")
    scale = packed.ls_scales(time, n_off, plan)
    f_day = plan.f_day
    kw = dict(normalization=plan.norm, scale=scale, device=device)
    if plan.nterms == 1 and plan.ls_method in ("fast", "fastchi2"):
        return _capi.ls_fast_peaks_batch(time, flux, n_off, f0=float(f_day[0]), df=float(f_day[1] - f_day[0]), M=M,
                                         want_power=want_power, want_peaks=want_peaks, out=out, absolute_time=True, **kw)
    trel = packed.rebase_times(time, n_off)
    if plan.nterms > 1 and plan.ls_method == "fastchi2":
        power = _capi.ls_fast_batch(trel, flux, n_off, f0=float(f_day[0]), df=float(f_day[1] - f_day[0]), M=M,
                                    nterms=plan.nterms, **kw)
    elif plan.exact is not None:
        power = _capi.ls_power_batch(trel, flux, n_off, f0=plan.exact[0], df=plan.exact[1], M=M, nterms=plan.nterms, **kw)
    else:
        power = _capi.ls_power_batch(trel, flux, n_off, frequency=f_day, nterms=plan.nterms, **kw)
    mx = am = None
    if want_peaks:
        mx, am = _capi.argmax_batch(power, device=device)
    if out is not None and want_power:
        out[...] = power
        power = out
    return (power if want_power else None), mx, am


def lombscargle_batch(lcs, frequency, normalization="amplitude", freq_unit=None, oversample_factor=None,
                      ls_method="fast", device=None, gather=True, nterms=1, out=None):
    """Lomb-Scargle power of every light curve on one shared frequency grid -> float64[len(lcs), M].
    Same result per target as ``LombScarglePeriodogram.from_lightcurve(lc, frequency=frequency, ...)``
    (``ls_method="fast"``: the reference's default FFT method; any other name: the exact kernels; ``nterms`` > 1
    with ``ls_method`` "chi2"/"fastchi2": the multi-term kernels), but planned per BATCH: the grid is examined once,
    the light curves are packed by one concatenation per column (``lcs``: a list of light curves — this package's or
    lightkurve's — or a ``LightCurveBatch``, whose arrays are used as they are).  ``out``: preallocated float64[B, M]
    (e.g. ``_capi.pinned_empty``) for the single-process result.
    With torch.distributed initialised, rank r computes a contiguous block of targets (balanced by cadence
    count) and, if ``gather``, the spectra are all-gathered so every rank returns all rows."""
    device = _resolve_device(device)
    plan = packed.ls_grid_plan(frequency, normalization, freq_unit, oversample_factor, ls_method, nterms)
    if gather and plan.nterms == 1 and plan.ls_method == "fast" and device_gather_available():
        return _lombscargle_fast_gather_on_device(lcs, plan, device)
    (time, flux), n_off, bounds = _local_packed(lcs, ("time", "flux"))
    power = _ls_power_packed(time, flux, n_off, plan, device, out=out if bounds is None else None)[0]
    return _finish(power, bounds, gather)


def _lombscargle_fast_gather_on_device(lcs, plan, device):
    """The multi-GPU form of ``lombscargle_batch`` for the default method with a RCCL group: this rank's block goes
    host -> HBM once, ``lk_ls_fast_peaks_batch_dev`` writes the spectra into a device tensor, the all-gather runs
    HBM -> xGMI -> HBM, and the full (B, M) result crosses PCIe once on the way out.  Tensors, stream and the lk_handle
    all belong to ONE device (``device``: the rank's own GPU), made current for the duration."""
    import torch
    (t_l, y_l), off, bounds = _local_packed(lcs, ("time", "flux"), pinned=False)
    t_l, y_l, off = packed.drop_nan_flux(t_l, y_l, off)
    if len(off) > 1 and np.diff(off).min() < 2:
        raise ValueError("The light curve needs at least two cadences to build a periodogram.")
    nb, M = len(off) - 1, len(plan.f_day)
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        d_pow = torch.empty((nb, M), dtype=torch.float64, device=dev)
        if nb:
            f_day = plan.f_day
            d_t = torch.from_numpy(packed.rebase_times(t_l, off)).to(dev)
            d_y = torch.from_numpy(np.ascontiguousarray(y_l)).to(dev)
            d_scale = torch.from_numpy(packed.ls_scales(t_l, off, plan)).to(dev)
            d_max = torch.empty(nb, dtype=torch.float64, device=dev)
            d_arg = torch.empty(nb, dtype=torch.int64, device=dev)
            h = _capi.Handle.get(device)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _capi.ls_fast_peaks_batch_dev(h, nb, off, d_t.data_ptr(), d_y.data_ptr(), 0, float(f_day[0]),
                                          float(f_day[1] - f_day[0]), M, True, True, plan.norm, d_scale.data_ptr(), 5,
                                          d_pow.data_ptr(), d_max.data_ptr(), d_arg.data_ptr(), stream)
        return all_gather_rows(d_pow, bounds).cpu().numpy()


def lombscargle_peaks_batch(lcs, frequency, normalization="amplitude", freq_unit=None, oversample_factor=None, device=None,
                            gather=True):
    """(max power, argmax) of the default-method (``ls_method="fast"``) periodogram of every light curve on one shared
    regular grid -> float64[len(lcs), 2] (column 1 holds the index).  The spectra never leave the GPU
    (lk_ls_fast_peaks_lc_batch with power = NULL) and with a process group only 16 B per target cross xGMI: this is the
    collective to use when ``Periodogram.max_power`` / ``frequency_at_max_power`` is what the pipeline keeps
    (reference periodogram.py:127-140) — ``lombscargle_batch(gather=True)`` makes every rank hold all B x M powers."""
    device = _resolve_device(device)
    plan = packed.ls_grid_plan(frequency, normalization, freq_unit, oversample_factor, "fast", 1)
    if plan.ls_method != "fast":
        raise ValueError("lombscargle_peaks_batch needs a regular frequency grid (the reference switches to 'slow')")
    (time, flux), n_off, bounds = _local_packed(lcs, ("time", "flux"))
    _pw, mx, am = _ls_power_packed(time, flux, n_off, plan, device, want_power=False, want_peaks=True)
    return _finish(np.column_stack([mx, am.astype(np.float64)]), bounds, gather)


def _bls_options(period, duration, objective, oversample):
    """The grid-level checks of ``BoxLeastSquaresPeriodogram.from_lightcurve`` / astropy ``BoxLeastSquares.power``
    (reference periodogram.py:1101-1112, astropy bls/core.py:277-327, 668-700), once per batch."""
    period = np.atleast_1d(np.asarray(period, dtype=np.float64))
    if duration is None:
        duration = [0.05, 0.10, 0.15, 0.20, 0.25, 0.33]
    duration = np.atleast_1d(np.asarray(duration, dtype=np.float64))
    if not np.all(np.isfinite(duration)):
        raise ValueError("`duration` parameter contains illegal nan or inf value(s)")
    if not np.all(np.isfinite(period)):
        raise ValueError("`period` parameter contains illegal nan or inf value(s)")
    if period.ndim != 1 or period.size == 0:
        raise ValueError("period must be 1-dimensional")
    if duration.ndim != 1 or duration.size == 0:
        raise ValueError("duration must be 1-dimensional")
    if np.min(period) <= np.max(duration):
        raise ValueError("The maximum transit duration must be shorter than the minimum period")
    try:
        oversample = int(oversample)
    except TypeError:
        raise ValueError("oversample must be an int, got {0}".format(oversample))
    if oversample < 1:
        raise ValueError("oversample must be greater than or equal to 1")
    objective = objective or "likelihood"
    if objective not in ["snr", "likelihood"]:
        raise ValueError("Unrecognized method '{0}'\nallowed methods are: {1}".format(objective, ["snr", "likelihood"]))
    return period, duration, objective, oversample


def bls_batch(lcs, period, duration=None, objective="likelihood", oversample=10, device=None, gather=True):
    """BLS power (and the other six statistics) of every light curve on one shared period grid.
    Returns float64[len(lcs), 7, nP] ordered as ``_capi.BLS_FIELDS`` (transit_time absolute, like the reference).
    ``lcs``: a list of light curves or a ``LightCurveBatch``; the per-target inputs (t - min t, y - median y, ivar) are
    built by vectorised passes over the packed arrays (``packed.bls_inputs``)."""
    device = _resolve_device(device)
    period, duration, objective, oversample = _bls_options(period, duration, objective, oversample)
    (time, flux, err), n_off, bounds = _local_packed(lcs, ("time", "flux", "flux_err"), prefix="bls")
    if len(n_off) == 1:
        return _finish(np.zeros((0, 7, len(period))), bounds, gather)
    t, y, w, off2, t_ref = packed.bls_inputs(time, flux, err, n_off)
    res = _capi.bls_batch(t, y, w, off2, period, duration, oversample, objective == "likelihood", device=device)
    out = np.stack([res[k] for k in _capi.BLS_FIELDS], axis=1)
    out[:, 4, :] += t_ref[:, None]
    return _finish(out, bounds, gather)


def bls_stats_batch(lcs, period, duration, transit_time, device=0):
    """``BoxLeastSquaresPeriodogram.compute_stats`` of one box per light curve (reference periodogram.py:1194-1229 over
    astropy compute_stats) for host light curves: ``lcs`` a list of light curves or a ``LightCurveBatch``; ``period`` /
    ``duration`` / ``transit_time`` (absolute) scalars or one value per light curve.  NaN-flux cadences are dropped and
    ivar = 1 / flux_err^2 (ones where the errors are not all finite), as for ``bls_batch``; the light curves must be sorted
    by time.  Returns the dict of ``DeviceBLSResult.compute_stats``.  Not sharded over ranks."""
    from .ingest import LightCurveBatch
    if isinstance(lcs, LightCurveBatch):
        time, flux, err, n_off = lcs.time, lcs.flux, lcs.flux_err, lcs.n_off
    else:
        (time, flux, err), n_off = packed.pack_columns(list(lcs), ("time", "flux", "flux_err"), pinned="auto", pool_prefix="blsstats")
    time, flux, n_off, err = packed.drop_nan_flux(time, flux, n_off, err)
    counts = np.diff(n_off)
    if len(counts) and counts.min() < 1:
        raise ValueError("a light curve of the batch has no finite flux")
    if not packed.check_sorted(time, n_off):
        raise ValueError("bls_stats_batch needs every light curve sorted by time")
    return _capi.bls_stats_batch(time, flux, packed.bls_ivar(flux, err, n_off), n_off, period, duration, transit_time, device=device)


def ls_model_batch(lcs, frequency, nterms=1, fit_mean=True, center_data=True, use_flux_err=False, keep_mean=True, want_model=True,
                   want_residual=False, device=0):
    """``LombScarglePeriodogram.model`` before its normalisation (reference periodogram.py:991-1018 over astropy
    ``LombScargle.model``) at one frequency [1/d] per light curve, for host light curves: ``lcs`` a list of light curves or a
    ``LightCurveBatch``; ``frequency`` a scalar or one value per light curve (NaN or <= 0: the light curve is skipped, status
    0).  NaN-flux cadences are dropped, as ``LombScarglePeriodogram.from_lightcurve`` drops them; weights are uniform, as
    lightkurve's, unless ``use_flux_err`` (then 1 / flux_err^2 where a light curve's errors are all finite).  Returns the dict
    of ``_capi.ls_model_batch`` plus ``n_off``, the offsets of the per-cadence arrays.  Not sharded over ranks."""
    from .ingest import LightCurveBatch
    if isinstance(lcs, LightCurveBatch):
        time, flux, err, n_off = lcs.time, lcs.flux, lcs.flux_err, lcs.n_off
    else:
        (time, flux, err), n_off = packed.pack_columns(list(lcs), ("time", "flux", "flux_err"), pinned="auto", pool_prefix="lsmodel")
    time, flux, n_off, err = packed.drop_nan_flux(time, flux, n_off, err)
    out = _capi.ls_model_batch(time, flux, err if use_flux_err else None, n_off, frequency, nterms, fit_mean, center_data, keep_mean,
                               want_model, want_residual, device=device)
    out["n_off"] = n_off
    return out


def fold_bin_batch(lcs, period, epoch_time=None, epoch_phase=0.0, wrap_phase=None, normalize_phase=False, time_bin_size=None,
                   time_bin_start=None, n_bins=None, bins=None, aggregate_func="mean", which="all", device=0):
    """``lc.fold(period, epoch_time, ...).bin(...)`` per light curve (reference lightcurve.py:1089-1214, 1558-1763), optionally
    of the odd or even cycles only, for host light curves: ``lcs`` a list of light curves or a ``LightCurveBatch``; ``period``
    / ``epoch_time`` / ``wrap_phase`` / ``time_bin_size`` / ``time_bin_start`` / ``n_bins`` scalars or one value per light
    curve.  The fused kernel (``lk_fold_bin_batch``: no sort, no folded copy) with the arguments and semantics of
    ``DeviceLightCurveBatch.fold_bin``; ``aggregate_func="mean"`` only.  Returns dict(phase, flux, flux_err, count, bin_off):
    light curve b's bins are ``[bin_off[b]:bin_off[b + 1]]``.  Not sharded over ranks."""
    from .ingest import LightCurveBatch
    if isinstance(lcs, LightCurveBatch):
        time, flux, err, n_off = lcs.time, lcs.flux, lcs.flux_err, lcs.n_off
    else:
        (time, flux, err), n_off = packed.pack_columns(list(lcs), ("time", "flux", "flux_err"), pinned="auto", pool_prefix="foldbin")
    return _capi.fold_bin_batch(time, flux, n_off, period, flux_err=err, epoch_time=epoch_time, epoch_phase=epoch_phase,
                                wrap_phase=wrap_phase, normalize_phase=normalize_phase, time_bin_size=time_bin_size,
                                time_bin_start=time_bin_start, n_bins=n_bins, bins=bins, aggregate_func=aggregate_func,
                                which=which, device=device)


def river_batch(lcs, period, epoch_time=None, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5, method="mean", bins=None,
                max_output_mb=4096, device=0):
    """River diagrams (cycle x phase images, the data behind ``plot_river`` of lightkurve 2.x) per light curve, for host light
    curves: ``lcs`` a list of light curves or a ``LightCurveBatch``; ``period`` / ``epoch_time`` / ``bins`` scalars or one value
    per light curve.  The arguments, definition and statuses of ``DeviceLightCurveBatch.river``, through ``lk_river_plan_batch`` /
    ``lk_river_batch``.  Returns the dict of ``_capi.river_batch``: ``river`` / ``count`` are lists of per-light-curve
    (n_cycles, n_bins) arrays.  ``method="sigma"`` needs errors: light curves without them carry NaN errors, which ``nansum``
    skips.  Not sharded over ranks."""
    from .ingest import LightCurveBatch
    if isinstance(lcs, LightCurveBatch):
        time, flux, err, n_off = lcs.time, lcs.flux, lcs.flux_err, lcs.n_off
    else:
        (time, flux, err), n_off = packed.pack_columns(list(lcs), ("time", "flux", "flux_err"), pinned="auto", pool_prefix="river")
    return _capi.river_batch(time, flux, n_off, period, flux_err=err, epoch_time=epoch_time, bin_points=bin_points,
                             minimum_phase=minimum_phase, maximum_phase=maximum_phase, method=method, bins=bins,
                             max_output_mb=max_output_mb, device=device)


def fill_gaps_batch(lcs, method="gaussian_noise", noise_std="auto", seed=0, first_target=0, stream_id=0, return_mask=False, device=0):
    """``lc.fill_gaps(method="gaussian_noise")`` of lightkurve 2.x per light curve, for host light curves: ``lcs`` a list of light
    curves (the reference's time path) or a ``LightCurveBatch`` (by cadence number when it carries them).  The arguments and
    semantics of ``DeviceLightCurveBatch.fill_gaps``, through ``lk_fill_gaps_plan_batch`` / ``lk_fill_gaps_batch``.  Returns the
    filled ``LightCurveBatch`` (with ``return_mask`` also the bool mask of its inserted cadences).  Not sharded over ranks."""
    from .ingest import LightCurveBatch
    if not isinstance(lcs, LightCurveBatch):
        lcs = LightCurveBatch.from_lightcurves(list(lcs))
    return lcs.fill_gaps(method=method, noise_std=noise_std, seed=seed, first_target=first_target, stream_id=stream_id,
                         return_mask=return_mask, device=device)


def periodogram_peaks(power, device=0):
    """(max_power[B], argmax[B]) of a B x M power matrix on the GPU (Periodogram.max_power / nanargmax)."""
    return _capi.argmax_batch(power, device=device)


def flatten_batch(lcs, window_length=101, polyorder=2, break_tolerance=5, niters=3, sigma=3, masks=None, device=0,
                  gather=True):
    """``LightCurve.flatten`` trends (reference lightcurve.py:943-1078) of every light curve, sharded over the ranks of the
    process group (every target is independent): rank r flattens a contiguous, cadence-balanced block in one
    ``lk_savgol_trend_batch`` call; with ``gather`` every rank returns the list of all trends (ragged rows travel
    NaN-padded), otherwise its own block's."""
    from .flatten import flatten_trend_batch
    lcs = list(lcs)
    masks = [None] * len(lcs) if masks is None else list(masks)
    if len(masks) != len(lcs):
        raise ValueError("masks must hold one entry (array or None) per light curve")
    pairs = list(zip(lcs, masks))

    def compute(local):
        if not local:
            return []
        return flatten_trend_batch([lc for lc, _ in local], window_length=window_length, polyorder=polyorder,
                                   break_tolerance=break_tolerance, niters=niters, sigma=sigma,
                                   masks=[m for _, m in local], device=device)

    return sharded_map_ragged(pairs, compute, [len(lc.time) for lc in lcs], gather=gather)


def estimate_cdpp_batch(lcs, transit_duration=13, savgol_window=101, savgol_polyorder=2, sigma=5.0, device=0, gather=True):
    """``LightCurve.estimate_cdpp`` (reference lightcurve.py:1764-1833; its caller loops over light curves,
    correctors/metrics.py:64-84) of every light curve -> float64[len(lcs)] in ppm, sharded over the ranks."""
    from .lightcurve import estimate_cdpp_batch as one_gpu
    lcs = list(lcs)

    def compute(local):
        if not local:
            return np.zeros((0, 1))
        return one_gpu(local, transit_duration=transit_duration, savgol_window=savgol_window,
                       savgol_polyorder=savgol_polyorder, sigma=sigma, device=device)[:, None]

    out = sharded_map(lcs, compute, costs=[len(lc.time) for lc in lcs], gather=gather)
    return out[:, 0]


def pld_correct_batch(cubes, gather=True, device=0, ragged_masks=False, **kwargs):
    """``PLDCorrector(tpf).correct(...)`` (reference correctors/pldcorrector.py:203-427) for a list of same-shaped cutouts,
    sharded over the ranks: rank r runs ``correctors.pldcorrector.pld_correct_batch`` (design matrices + regression, two GPU
    calls) on its block.  ``ragged_masks`` goes to every rank's shard (PLD / background masks of different sizes per cutout);
    masks given as bool (B, ny, nx) arrays are split with the cutouts.  Returns (corrected_flux[B, N], outlier_mask[B, N]) — all
    B rows on every rank with ``gather``."""
    from .correctors.pldcorrector import _per_cutout_masks, pld_correct_batch as one_gpu
    cubes = list(cubes)
    mask_names = ("aperture_mask", "pld_aperture_mask", "background_aperture_mask")
    per = {k: _per_cutout_masks(kwargs[k], len(cubes), cubes[0].shape[1:]) for k in mask_names if k in kwargs and cubes}
    per = {k: m for k, m in per.items() if m is not None}
    if per:                                   # a shard takes its own rows of the per-cutout masks: items carry their index
        cubes = list(enumerate(cubes))

    def compute(local):
        if not local:
            return np.zeros((0, 2, 0))
        kw = dict(kwargs)
        if per:
            rows = [i for i, _ in local]
            local = [c for _, c in local]
            kw.update({k: m[rows] for k, m in per.items()})
        flux, outl = one_gpu(local, device=device, ragged_masks=ragged_masks, **kw)
        return np.stack([flux, outl.astype(np.float64)], axis=1)

    dist_on = False
    try:
        import torch.distributed as dist
        dist_on = dist.is_available() and dist.is_initialized()
    except ImportError:
        pass
    if dist_on and gather:
        # an empty local block has no cadence count of its own: take it from the batch (same-shaped cutouts)
        from .correctors.pldcorrector import PLDCorrector
        first = (cubes[0][1] if per else cubes[0]) if cubes else None
        ap0 = per["aperture_mask"][0] if "aperture_mask" in per else kwargs.get("aperture_mask", "all")
        n = len(PLDCorrector(first, aperture_mask=ap0).lc) if cubes else 0

        def compute_n(local):
            return compute(local) if local else np.zeros((0, 2, n))

        out = sharded_map(cubes, compute_n, gather=True)
    else:
        out = sharded_map(cubes, compute, gather=gather)
    return out[:, 0], out[:, 1] != 0.0


def difference_images_batch(cubes, period, transit_time, duration, device=0, **kwargs):
    """``PixelCube.difference_image`` of every cutout, for host cutouts: ``cubes`` a list of same-shaped float32 ``PixelCube``s,
    ``period`` / ``transit_time`` / ``duration`` scalars or one value per cutout.  One upload (``DevicePixelCubeBatch.from_cubes``),
    then ``DevicePixelCubeBatch.difference_images`` with its keywords and its dict of host arrays.  Not sharded over ranks."""
    from .device import DevicePixelCubeBatch
    return DevicePixelCubeBatch.from_cubes(list(cubes), device=device).difference_images(period, transit_time, duration, **kwargs)


def amplitude_images_batch(cubes, frequency, device=0, **kwargs):
    """``PixelCube.amplitude_image`` of every cutout, for host cutouts: ``cubes`` a list of same-shaped float32 ``PixelCube``s,
    ``frequency`` a scalar or one value per cutout.  One upload (``DevicePixelCubeBatch.from_cubes``), then
    ``DevicePixelCubeBatch.amplitude_images`` with its keywords and its dict of host arrays.  Not sharded over ranks."""
    from .device import DevicePixelCubeBatch
    return DevicePixelCubeBatch.from_cubes(list(cubes), device=device).amplitude_images(frequency, **kwargs)


def psf_photometry_batch(cubes, star_col, star_row, sigma=None, device=0, **kwargs):
    """``PixelCube.psf_photometry`` of every cutout, for host cutouts: ``cubes`` a list of same-shaped float32 ``PixelCube``s,
    ``star_col`` / ``star_row`` [S] or [B, S] (NaN = no star), ``sigma`` a scalar, a pair or [B, 2] — or ``prf=`` a
    ``TabulatedPRF`` (and ``prf_index=``) in its place.  One upload
    (``DevicePixelCubeBatch.from_cubes``), then ``DevicePixelCubeBatch.psf_photometry`` with its keywords; returns its
    ``(lcs, info)``: the resident light curves, one per star, and ``info`` as host arrays unless ``to_host=False`` is passed.
    Not sharded over ranks."""
    from .device import DevicePixelCubeBatch
    kwargs.setdefault("to_host", True)
    return DevicePixelCubeBatch.from_cubes(list(cubes), device=device).psf_photometry(star_col, star_row, sigma, **kwargs)


def psf_fit_batch(cubes, star_col, star_row, sigma=None, device=0, **kwargs):
    """``PixelCube.psf_fit`` of every cutout, for host cutouts: PSF photometry with one common pointing shift per cadence fitted
    next to the fluxes.  ``cubes``, ``star_col`` / ``star_row`` and ``sigma`` — or ``prf=`` a ``TabulatedPRF`` (and
    ``prf_index=``) in its place — as in ``psf_photometry_batch``.  One upload
    (``DevicePixelCubeBatch.from_cubes``), then ``DevicePixelCubeBatch.psf_fit`` with its keywords; returns its ``(lcs,
    info)``, ``info`` as host arrays unless ``to_host=False`` is passed.  Not sharded over ranks."""
    from .device import DevicePixelCubeBatch
    kwargs.setdefault("to_host", True)
    return DevicePixelCubeBatch.from_cubes(list(cubes), device=device).psf_fit(star_col, star_row, sigma, **kwargs)


def psf_width_batch(cubes, star_col, star_row, sigma0, device=0, **kwargs):
    """``PixelCube.psf_width`` of every cutout, for host cutouts: the PSF width (sigma_col, sigma_row) of each cutout fitted on
    all its cadences (``DESIGN.md`` §5h).  ``cubes``: ``PixelCube``s of one (N, ny, nx) with float32 flux; they go up once
    (``DevicePixelCubeBatch.from_cubes``), then ``DevicePixelCubeBatch.psf_width`` with its keywords; returns its dict."""
    from .device import DevicePixelCubeBatch
    return DevicePixelCubeBatch.from_cubes(list(cubes), device=device).psf_width(star_col, star_row, sigma0, **kwargs)


def psf_positions_batch(cubes, star_col, star_row, sigma, device=0, **kwargs):
    """``PixelCube.psf_positions`` of every cutout, for host cutouts: the (column, row) of each fitted star of each cutout, fitted
    on all its cadences at given shifts and width (``DESIGN.md`` §5i).  ``cubes``: ``PixelCube``s of one (N, ny, nx) with float32
    flux; they go up once (``DevicePixelCubeBatch.from_cubes``), then ``DevicePixelCubeBatch.psf_positions`` with its keywords;
    returns its dict."""
    from .device import DevicePixelCubeBatch
    return DevicePixelCubeBatch.from_cubes(list(cubes), device=device).psf_positions(star_col, star_row, sigma, **kwargs)


def pixel_periodograms_batch(cubes, frequency, device=0, **kwargs):
    """``PixelCube.pixel_periodogram`` of every cutout, for host cutouts: ``cubes`` a list of same-shaped float32 ``PixelCube``s,
    ``frequency`` one grid shared by all.  One upload (``DevicePixelCubeBatch.from_cubes``), then
    ``DevicePixelCubeBatch.pixel_periodograms`` with its keywords and its dict of host arrays.  Not sharded over ranks."""
    from .device import DevicePixelCubeBatch
    return DevicePixelCubeBatch.from_cubes(list(cubes), device=device).pixel_periodograms(frequency, **kwargs)


def subtract_background_batch(cubes, background=None, aperture_mask="background", device=0, to_host=True):
    """``PixelCube.subtract_background`` of every cutout, for host cutouts: ``cubes`` a list of same-shaped float32
    ``PixelCube``s, ``background`` None (each cutout's own estimate over ``aperture_mask``) or a (B, N) array.  One upload
    (``DevicePixelCubeBatch.from_cubes``), then ``DevicePixelCubeBatch.subtract_background``; returns the subtracted
    ``PixelCube``s, or the resident batch with ``to_host=False``.  Not sharded over ranks."""
    from .device import DevicePixelCubeBatch
    out = DevicePixelCubeBatch.from_cubes(list(cubes), device=device).subtract_background(background, aperture_mask)
    return out.to_host() if to_host else out


def regression_correct_batch(lcs, design_matrices, cadence_masks=None, sigma=5, niters=5, device=0, gather=True):
    """``RegressionCorrector(lc).correct(dm)`` (reference correctors/regressioncorrector.py:191-309) for many light curves
    whose design matrices share their column count K: one ``lk_regress_batch`` call per rank over its block (Gram on the
    fp64 matrix cores, solve, 5-sigma clipping loop per target).  Returns (corrected_flux list, coefficients[B, K],
    outlier_mask list); with ``gather`` for all targets on every rank."""
    from .correctors.designmatrix import DesignMatrix, DesignMatrixCollection
    lcs, dms = list(lcs), list(design_matrices)
    if len(dms) != len(lcs):
        raise ValueError("one design matrix (collection) per light curve")
    for d in dms:
        if not isinstance(d, (DesignMatrix, DesignMatrixCollection)):
            raise ValueError("design_matrix_collection must be a DesignMatrix or DesignMatrixCollection")
    # shapes and priors are checked for every target; the reference's low-rank WARNING (an SVD per matrix on the host,
    # designmatrix.py:306-337 — ~50 ms per target, i.e. minutes per 1000 targets) is left to the per-object path
    dms = [d if isinstance(d, DesignMatrixCollection) else DesignMatrixCollection([d], validate_rank=False) for d in dms]
    for d in dms:
        d.validate(rank=False)
    K = dms[0].X.shape[1] if dms else 0
    if any(d.X.shape[1] != K for d in dms):
        raise ValueError("regression_correct_batch needs design matrices with the same number of columns")
    cms = [None] * len(lcs) if cadence_masks is None else list(cadence_masks)
    lens = [len(lc.time) for lc in lcs]
    trip = list(zip(lcs, dms, cms))

    def compute(local):
        # one padded row per target: [flux - model (n), outlier (n), coefficients (K)], NaN beyond n
        if not local:
            return []
        X = np.concatenate([d.X for _, d, _ in local])
        y = np.concatenate([np.asarray(lc.flux, dtype=np.float64) for lc, _, _ in local])
        ns = [len(lc.time) for lc, _, _ in local]
        off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        errs = [np.asarray(lc.flux_err, dtype=np.float64) for lc, _, _ in local]
        err = None if all(np.all(~np.isfinite(e)) for e in errs) else np.concatenate(errs)
        cm = np.concatenate([np.ones(n, bool) if c is None else np.asarray(c, dtype=bool) for (_, _, c), n in zip(local, ns)])
        mu = np.stack([d.prior_mu for _, d, _ in local])
        sg = np.stack([d.prior_sigma for _, d, _ in local])
        has_prior = np.any(np.isfinite(sg)) or np.any(mu != 0)
        res = _capi.regress_batch(X, y, off, err=err, cadence_mask=cm, prior_mu=mu if has_prior else None,
                                  prior_sigma=sg if has_prior else None, sigma=sigma, niters=niters, device=device)
        rows = []
        for i, n in enumerate(ns):
            a, b = int(off[i]), int(off[i + 1])
            rows.append(np.concatenate([y[a:b] - res["model"][a:b], res["outlier_mask"][a:b].astype(np.float64),
                                        res["coefficients"][i]]))
        return rows

    rows = sharded_map_ragged(trip, compute, [2 * n + K for n in lens], costs=[n * K * K for n in lens] if K else None,
                              gather=gather)
    if not gather:
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                b = shard_bounds(len(lcs), dist.get_world_size(), [n * K * K for n in lens] if K else lens)
                lens = lens[int(b[dist.get_rank()]):int(b[dist.get_rank() + 1])]
        except ImportError:
            pass
    flux = [r[:n] for r, n in zip(rows, lens)]
    outl = [r[n:2 * n] != 0.0 for r, n in zip(rows, lens)]
    coef = np.stack([r[2 * n:2 * n + K] for r, n in zip(rows, lens)]) if rows else np.zeros((0, K))
    return flux, coef, outl


def cbv_correct_batch(lcs, cbvs, cadenceno=None, cbv_indices=np.arange(1, 9), alpha=1e-20, ext_dm=None, cadence_masks=None, sigma=5,
                      niters=5, device=0, cbv_time=None, gap_indicators=None, extrapolate=False):
    """``CBVCorrector(lc, cbvs.align(lc)).correct_gaussian_prior(cbv_indices, alpha, ext_dm, cadence_mask)`` for many host
    light curves that share the basis vectors of one channel but keep different cadences: ``cbvs`` (Nx, n_vectors) lives on
    the cadence grid ``cadenceno`` (Nx, strictly increasing) and every light curve carries its own ``cadenceno`` column.
    Cadences that are not on the grid are dropped, as ``align`` drops them; X goes to the device ONCE
    (``lk_regress_shared_rows_batch``), no stacked copy per target exists.  ``alpha``: scalar (0: no prior) or one
    penalty per target.  Returns (corrected_flux list, coefficients[B, K], outlier_mask list, kept list): ``kept[b]`` is the
    bool mask over light curve b's cadences of those that are on the grid (the others have no corrected flux).  One
    process, one device: a resident ``DeviceLightCurveBatch.cbv_correct(cadenceno=)`` is the route that scales.

    ``cbv_time`` (Nx,) instead of ``cadenceno``: ``CBVCorrector(lc, interpolate_cbvs=True, extrapolate_cbvs=extrapolate)`` —
    the light curves need no cadence numbers, the basis vectors are interpolated to each one's times on the device
    (``DeviceLightCurveBatch.cbv_correct(cbv_time=, gap_indicators=, extrapolate=)``, which this call goes through);
    ``kept[b]`` marks the cadences inside the CBVs' span (all of them with ``extrapolate``)."""
    from .device import DeviceLightCurveBatch, _alpha_per_target, _cbv_columns
    lcs = list(lcs)
    B = len(lcs)
    if (cadenceno is None) == (cbv_time is None):
        raise ValueError("cbv_correct_batch: pass `cadenceno` (the cadence numbers of the rows of cbvs) or `cbv_time` (their times)")
    if cbv_time is not None:
        if B == 0:
            return [], np.zeros((0, _cbv_columns(cbvs, cbv_indices, None).shape[1])), [], []
        col = lambda lc, name: np.asarray(getattr(getattr(lc, name), "value", getattr(lc, name)), dtype=np.float64)
        ts, ys, es = ([col(lc, name) for lc in lcs] for name in ("time", "flux", "flux_err"))
        off = np.concatenate([[0], np.cumsum([len(t) for t in ts])]).astype(np.int64)
        cms = None
        if cadence_masks is not None:
            cms = np.concatenate([np.ones(len(t), bool) if c is None else np.asarray(c, dtype=bool)
                                  for c, t in zip(cadence_masks, ts)])
        dev = DeviceLightCurveBatch.from_arrays(np.concatenate(ts), np.concatenate(ys), np.concatenate(es), off, device=device)
        flux, outl, coef = dev.cbv_correct(cbvs, cbv_indices=cbv_indices, alpha=alpha, ext_dm=ext_dm, cadence_mask=cms, sigma=sigma,
                                           niters=niters, to_host=True, cbv_time=cbv_time, gap_indicators=gap_indicators,
                                           extrapolate=extrapolate)
        x = np.asarray(cbv_time, dtype=np.float64)
        knots = x if gap_indicators is None else x[np.asarray(gap_indicators) == 0]
        kept = [np.ones(len(t), bool) if extrapolate else (t >= knots[0]) & (t <= knots[-1]) for t in ts]
        return flux, coef, outl, kept
    X = _cbv_columns(cbvs, cbv_indices, ext_dm)
    grid = np.asarray(cadenceno)
    if grid.shape != (X.shape[0],) or not np.issubdtype(grid.dtype, np.integer) or np.any(np.diff(grid) <= 0):
        raise ValueError("cadenceno must be %d strictly increasing integers, one per row of cbvs" % X.shape[0])
    alphas = None if np.ndim(alpha) == 0 else _alpha_per_target(alpha, B)
    cms = [None] * B if cadence_masks is None else list(cadence_masks)
    rows, ys, errs, cmk, kept = [], [], [], [], []
    for lc, c in zip(lcs, cms):
        cad = np.asarray(getattr(lc, "cadenceno"))
        cad = np.asarray(getattr(cad, "value", cad))
        if not np.issubdtype(cad.dtype, np.integer) or cad.shape != (len(lc.time),):
            raise ValueError("every light curve needs an integer cadenceno column, one entry per cadence")
        if np.any(np.diff(cad) <= 0):
            raise ValueError("every light curve's cadence numbers must be strictly increasing")
        r = np.searchsorted(grid, cad)
        ok = (r < grid.size) & (grid[np.minimum(r, grid.size - 1)] == cad)
        kept.append(ok), rows.append(r[ok])
        ys.append(np.asarray(getattr(lc.flux, "value", lc.flux), dtype=np.float64)[ok])
        errs.append(np.asarray(getattr(lc.flux_err, "value", lc.flux_err), dtype=np.float64)[ok])
        cmk.append(np.ones(int(ok.sum()), bool) if c is None else np.asarray(c, dtype=bool)[ok])
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    if B == 0:
        return [], np.zeros((0, X.shape[1])), [], []
    y, err = np.concatenate(ys), np.concatenate(errs)
    mu = sg = None
    if alphas is not None or alpha != 0.0:
        mu, sg = _capi.ridge_prior_rows_batch(err, off, X.shape[1], alpha if alphas is None else alphas, device=device)
    res = _capi.regress_shared_rows_batch(X, y, off, np.concatenate(rows), err=err, cadence_mask=np.concatenate(cmk), prior_mu=mu,
                                          prior_sigma=sg, sigma=sigma, niters=niters, device=device)
    cut = off[1:-1]
    return np.split(y - res["model"], cut), res["coefficients"], np.split(res["outlier_mask"], cut), kept
