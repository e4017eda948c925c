"""Host side of the phase-binned folded light curve (``lc.fold(...).bin(...)``): argument checks and the bin layout.

Pure numpy, no GPU: the device (``lk_fold_bin_plan_batch*``) reports eight numbers per target, and this module turns them and
the caller's arguments into what ``lk_phase_bin_batch_dev`` and ``lk_fold_bin_batch*`` take — start, bin size, number of bins
and the edges of every target.  Both device routes (``DeviceFoldedBatch.bin`` and the fused ``fold_bin``) go through
``phase_bin_layout``, so their layouts are the same by construction.

Semantics: ``LightCurve.bin`` (reference lightcurve.py:1558-1763) over astropy 4.3.1 ``aggregate_downsample``
(timeseries/downsample.py:60-130) applied to the phase column, as ``lk_bin_batch`` applies them to time: relative time
``r = (phase - start) * 86400``; edges = numpy's running sum of the bin size; a slot belongs to bin k when
``edges[k] < r <= edges[k+1]`` (``r == 0``: bin 0) and ``r < edges[n_bins]``; ``n_bins`` defaults to
``ceil(r_last / size)``, so a last slot exactly on the last edge is dropped, as in the reference."""
import numpy as np

NPLAN = 8                       # LK_FOLD_BIN_NPLAN (include/lkhip.h)
LDS_BINS = 1024                 # LK_FOLD_BIN_LDS_BINS: bins per target the fused kernel accumulates in LDS (more: a global slab)
ONE_NS = 1e-9 / 86400.0         # [d]
WHICH = {"all": 0, "odd": 1, "even": 2}
AGGREGATES = ("mean", "median")


def check_bin_arguments(time_bin_size=None, n_bins=None, bins=None, aggregate_func="mean", which="all"):
    """Validate what ``bin`` / ``fold_bin`` were given -> (aggregate_func, which code).  ``ValueError`` for ``bins`` together
    with ``time_bin_size`` or ``n_bins``, a ``bins`` below 1, an unknown ``aggregate_func`` or ``which``."""
    if bins is not None:
        if time_bin_size is not None or n_bins is not None:
            raise ValueError("bins cannot be given together with time_bin_size or n_bins")
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
            raise ValueError("bins must be a positive integer (got %r)" % (bins,))
    if aggregate_func is None:
        aggregate_func = "mean"
    if aggregate_func not in AGGREGATES:
        raise ValueError("aggregate_func must be 'mean' or 'median' (got %r)" % (aggregate_func,))
    if which not in WHICH:
        raise ValueError("which must be 'all', 'odd' or 'even' (got %r)" % (which,))
    return aggregate_func, WHICH[which]


def _per_target(value, B, name):
    try:
        return np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float64), (B,))).copy()
    except ValueError:
        raise ValueError("%s must be a scalar or one value per light curve" % name)


def count_from(time_bin_start, bins, B):
    """The threshold of the plan's count (slot [2]): with ``bins=`` and a given start the reference counts the slots whose
    phase is >= start - 1 ns; otherwise every slot counts (None)."""
    if bins is None or time_bin_start is None:
        return None
    return _per_target(time_bin_start, B, "time_bin_start") - ONE_NS


def bins_to_size(phase_first_to_last, i, bins):
    """The v1-compatibility form ``bin(bins=)``: time_bin_size [d] = (phase_last - start) * i / ((i - 1) * bins), with i the
    number of slots whose phase is >= start - 1 ns.  (Stated from knowledge of the reference, whose source was not at hand:
    the formula as written here is the contract.)"""
    i = np.asarray(i, dtype=np.float64)
    if np.any(i < 2):
        raise ValueError("bins= needs at least two cadences at or after the start in every light curve")
    return np.asarray(phase_first_to_last, dtype=np.float64) * i / ((i - 1) * bins)


def phase_bin_layout(counts, plan, time_bin_size=None, time_bin_start=None, n_bins=None, bins=None):
    """-> dict(start[B] [phase units], size[B] [d], size_sec[B], bin_off[B + 1], edges[bin_off[B] + B] [s]) from the cadence
    counts and the device's plan (``plan[b]``: smallest phase, largest phase, slots >= count_from, ...).  Sizes and starts are
    scalars or one value per light curve; the edges of target b are ``edges[bin_off[b] + b : bin_off[b + 1] + b + 1]``, the
    running sum ``np.cumsum([0, size_sec, size_sec, ...])`` of ITS size.  A light curve without cadences gets no bins."""
    counts = np.asarray(counts, dtype=np.int64)
    B = counts.size
    plan = np.asarray(plan, dtype=np.float64).reshape(B, NPLAN)
    has = (counts > 0) & np.isfinite(plan[:, 0])
    first, last = np.where(has, plan[:, 0], 0.0), np.where(has, plan[:, 1], 0.0)
    start = first.copy() if time_bin_start is None else _per_target(time_bin_start, B, "time_bin_start")
    start[~has] = 0.0
    if not np.all(np.isfinite(start)):
        raise ValueError("time_bin_start must be finite")
    if bins is not None:
        size = bins_to_size(last - start, plan[:, 2], int(bins))
    else:
        size = _per_target(0.5 if time_bin_size is None else time_bin_size, B, "time_bin_size")
    size_sec = size * 86400.0
    if np.any(has & ~(size_sec > 0)) or not np.all(np.isfinite(size_sec[has])):
        raise ValueError("time_bin_size must be positive")
    size_sec[~has] = 1.0
    if n_bins is None:
        with np.errstate(invalid="ignore"):
            nb = np.maximum(0, np.ceil((last - start) * 86400.0 / size_sec))
    else:
        nb = _per_target(n_bins, B, "n_bins")
        if np.any(nb < 0) or np.any(nb != np.floor(nb)):
            raise ValueError("n_bins must be a non-negative integer")
    nb = np.where(has, nb, 0).astype(np.int64)
    bin_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(nb, out=bin_off[1:])
    edges = np.zeros(int(bin_off[-1]) + B, dtype=np.float64)
    width = int(nb.max()) + 1 if B else 0
    if B and B * width <= 4 * edges.size:
        # one padded table: row b is the sequential sum np.cumsum([0, size_b, size_b, ...]), of which target b keeps n_bins_b + 1
        e = np.empty((B, width), dtype=np.float64)
        e[:, 0] = 0.0
        e[:, 1:] = size_sec[:, None]
        edges[:] = np.cumsum(e, axis=1)[np.arange(width)[None, :] <= nb[:, None]]
    else:
        for b in range(B):
            lo = int(bin_off[b]) + b
            edges[lo:lo + int(nb[b]) + 1] = np.cumsum(np.hstack([0.0, np.repeat(size_sec[b], int(nb[b]))]))
    return dict(start=start, size=size, size_sec=size_sec, bin_off=bin_off, edges=edges)
