"""Inputs and pure numpy restatements for the phase-binned folded light curve (tests/test_foldbin_cpu.py,
tests/test_foldbin_gpu.py).  Nothing here imports the package under test; the fold itself is ``oracle.np_oracle.fold``.

Restated: ``FoldedLightCurve.cycle`` (``fold_cycle``), ``lc.fold(...).bin(...)`` with the semantics of ``LightCurve.bin`` over
astropy 4.3.1 ``aggregate_downsample`` on the phase column (``phase_bin_reference``) and the v1-compatibility ``bins=`` form
(``bins_to_size``)."""
import functools
import warnings

import numpy as np

from oracle import np_oracle as O

ONE_NS = 1e-9 / 86400.0     # [d]


# ------------------------------------------------------------------------------------------------ restatements
def fold_cycle(time_original, period, phase_sorted, epoch_time=None):
    """floor((t - (e - P/2)) / P) minus its minimum; e = the epoch given to fold, else the smallest folded phase."""
    t = np.asarray(time_original, float)
    if t.size == 0:
        return np.zeros(0, dtype=np.int64)
    e = float(epoch_time) if epoch_time is not None else float(np.min(phase_sorted))
    c = np.floor((t - (e - period / 2.0)) / period).astype(np.int64)
    return c - c.min()


def bins_to_size(phase_last, start, i, bins):
    """time_bin_size [d] of ``bin(bins=)``: (phase_last - start) * i / ((i - 1) * bins), i = slots with phase >= start - 1 ns."""
    if i < 2:
        raise ValueError("bins= needs at least two cadences")
    return (phase_last - start) * i / ((i - 1) * bins)


def phase_bin_reference(phase_sorted, flux, flux_err, cycle, size=None, start=None, n_bins=None, bins=None, aggregate="mean",
                        which="all"):
    """-> dict(phase, flux, flux_err, count, start, size): bin centres, aggregated flux, rmse of the errors (nanstd of the flux
    when the light curve has no finite error), slots per bin.  The layout comes from ALL slots, ``which`` only restricts what is
    aggregated."""
    ph = np.asarray(phase_sorted, float)
    f = np.asarray(flux, float)
    if ph.size == 0:
        z = np.zeros(0)
        return dict(phase=z, flux=z, flux_err=z, count=np.zeros(0, dtype=np.int32), start=0.0, size=size)
    e = None if flux_err is None else np.asarray(flux_err, float)
    start = float(ph[0]) if start is None else float(start)
    if bins is not None:
        assert size is None and n_bins is None
        size = bins_to_size(float(ph[-1]), start, int(np.sum(ph >= start - ONE_NS)), bins)
    elif size is None:
        size = 0.5
    size_sec = size * 86400.0
    rel = (ph - start) * 86400.0
    nb = int(n_bins) if n_bins is not None else max(0, int(np.ceil(rel[-1] / size_sec)))
    edges = np.cumsum(np.hstack([0.0, np.repeat(size_sec, nb)]))
    keep = (rel >= edges[0]) & (rel < edges[-1])
    idx = np.searchsorted(edges, rel) - 1          # edges[idx] < rel <= edges[idx + 1]
    idx[rel == edges[0]] = 0
    parity = {"all": np.ones(ph.size, bool), "odd": np.asarray(cycle) % 2 == 1, "even": np.asarray(cycle) % 2 == 0}[which]
    sel = keep & parity
    has_err = e is not None and bool(np.any(np.isfinite(e)))
    out_f, out_e, cnt = np.full(nb, np.nan), np.full(nb, np.nan), np.zeros(nb, dtype=np.int32)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(nb):
            m = sel & (idx == k)
            cnt[k] = m.sum()
            if not cnt[k]:
                continue
            out_f[k] = np.nanmean(f[m]) if aggregate == "mean" else np.nanmedian(f[m])
            if has_err:
                x = e[m]
                out_e[k] = np.sqrt(np.nansum(x ** 2) / np.sum(np.isfinite(x))) if np.any(np.isfinite(x)) else np.nan
            else:
                out_e[k] = np.nanstd(f[m])
    return dict(phase=start + (edges[:-1] + size_sec / 2.0) / 86400.0, flux=out_f, flux_err=out_e, count=cnt, start=start, size=size)


# ------------------------------------------------------------------------------------------------ cases
LENGTHS = (5000, 1, 63, 0, 64, 65, 1500)      # (the empty light curve sits in the middle: neither first nor last)
EXACT = 4                                      # index of the light curve on binary fractions
COMMENSURATE = 6
NANSTD = 2                                     # index of the light curve whose errors are all NaN


def _target(b, n):
    rng = np.random.RandomState(100 + b)
    if b == EXACT:          # times on multiples of 2^-4 d (also of 2^-10), period 1: phases are multiples of 1/16 in [-1/2, 1/2)
        time, period = 10.0 + np.arange(n) * 2.0 ** -4, 1.0
    elif b == COMMENSURATE:  # period = 8 cadences exactly: eight distinct phases, every other bin stays empty
        time, period = 50.0 + np.arange(n) * 2.0 ** -6, 8 * 2.0 ** -6
    elif n == 65:           # exactly one cycle: the period is longer than the baseline
        time, period = 3.0 + 0.02 * np.arange(n) + 1e-4 * rng.rand(n), 1.7
    else:                   # about 20 cycles
        time = 7.0 + 0.02 * np.arange(n) + 1e-4 * rng.rand(n)
        period = max(0.02 * max(n, 2) / 20.03, 0.0131)
    flux = 1.0 + 1e-3 * rng.randn(n) - 0.01 * (np.abs(((time - time[0]) / period + 0.5) % 1.0 - 0.5) < 0.04 if n else 0.0)
    err = 1e-3 * (1.0 + 0.2 * rng.rand(n))
    flux[::37] = np.nan                       # NaN flux scattered through the batch
    err[5::41] = np.nan
    if b == COMMENSURATE:
        flux[3::8] = np.nan                   # one phase value, hence one bin, whose flux is all NaN
    if b == NANSTD:
        err[:] = np.nan                       # no finite error: the nanstd form
    for a in (time, flux, err):
        a.setflags(write=False)
    return dict(time=time, flux=flux, flux_err=err, period=float(period))


@functools.lru_cache(maxsize=None)
def batch():
    """The light curves of the GPU test, read-only: list of dict(time, flux, flux_err, period)."""
    return tuple(_target(b, n) for b, n in enumerate(LENGTHS))


@functools.lru_cache(maxsize=None)
def folded(epoch_given=False, with_err=True):
    """The reference fold of every light curve of ``batch()`` (epoch_time: the first time, passed explicitly or not — the phases
    are the same, the cycle's epoch is not): list of dict(phase, order, flux, flux_err, cycle, time_original)."""
    out = []
    for tg in batch():
        t, P = tg["time"], tg["period"]
        if t.size == 0:
            z = np.zeros(0)
            out.append(dict(phase=z, order=np.zeros(0, dtype=np.int64), flux=z, flux_err=z if with_err else None,
                            cycle=np.zeros(0, dtype=np.int64), time_original=z))
            continue
        phase, order, _ = O.fold(t, P, t[0])
        cyc = fold_cycle(t[order], P, phase, t[0] if epoch_given else None)
        out.append(dict(phase=phase, order=order, flux=tg["flux"][order], flux_err=tg["flux_err"][order] if with_err else None,
                        cycle=cyc, time_original=t[order]))
    return out


def per_target_sizes():
    """(time_bin_size[B], time_bin_start[B]) for the per-target form: the light curve on binary fractions gets size 1/8 from
    -1/2, so every other of its phases (multiples of 1/16) falls exactly on an edge (in seconds: multiples of 5400 against
    edges at multiples of 10800, all exact); the others get sizes of their own from their smallest phase."""
    sizes, starts = [], []
    for b, (tg, fo) in enumerate(zip(batch(), folded())):
        if b == EXACT:
            sizes.append(0.125), starts.append(-0.5)
        else:
            sizes.append(tg["period"] / (17.0 + b)), starts.append(float(fo["phase"][0]) if fo["phase"].size else 0.0)
    return np.array(sizes), np.array(starts)
