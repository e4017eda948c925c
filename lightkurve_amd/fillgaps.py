"""Argument handling shared by the ``fill_gaps`` / ``stitch`` front ends (``DeviceLightCurveBatch``, ``LightCurveBatch``): what
the reference's ``LightCurve.fill_gaps`` and ``LightCurveCollection.stitch`` decide in Python before any array work.  Nothing
here touches the device."""
import numpy as np

METHODS = ("gaussian_noise",)
NOISE_MODES = ("auto", "std", "cdpp")
QUALITY_INSERTED = 65536      # the flag of an inserted cadence (lightkurve 2.x fill_gaps)


def check_fill_gaps(method, by, has_cadenceno, noise_std, noise_mean, meta):
    """-> (by_cadenceno, mode, noise_std array or None, noise_mean array or None); ``mode`` is "std", "cdpp" or "given"."""
    B = len(meta)
    if method not in METHODS:
        raise NotImplementedError("Method {} is not implemented: fill_gaps knows {}".format(method, list(METHODS)))
    if by not in ("auto", "time", "cadenceno"):
        raise ValueError("by must be 'auto', 'time' or 'cadenceno' (got %r)" % (by,))
    if by == "cadenceno" and not has_cadenceno:
        raise ValueError("fill_gaps(by='cadenceno') needs a batch that carries cadence numbers (from_fits, from_arrays(cadenceno=))")
    by_cad = has_cadenceno if by == "auto" else by == "cadenceno"
    std = None
    if isinstance(noise_std, str):
        if noise_std not in NOISE_MODES:
            raise ValueError("noise_std must be one of %s or an array of one value per light curve (got %r)"
                             % (list(NOISE_MODES), noise_std))
        mode = noise_std
        if mode == "auto":
            mode = "cdpp" if B > 0 and all(bool(m.get("NORMALIZED")) for m in meta) else "std"
    else:
        std = _per_target(noise_std, B, "noise_std")
        mode = "given"
    mean = None if noise_mean is None else _per_target(noise_mean, B, "noise_mean")
    return by_cad, mode, std, mean


def _per_target(a, B, name):
    a = np.asarray(a, dtype=np.float64)
    if a.shape != (B,):
        raise ValueError("%s must hold one value per light curve: shape (%d,), got %s" % (name, B, a.shape))
    return np.ascontiguousarray(a)


def noise_arrays(stats, mode, std, mean, cdpp):
    """The per-target (noise_mean, noise_std) the fill takes: ``stats`` (B, 4) = the plan's m, mu, sd, n_inserted; ``cdpp``: a
    callable -> ppm[B], called for mode "cdpp" only (a NaN CDPP falls back to sd, as the reference's except branch)."""
    stats = np.asarray(stats, dtype=np.float64).reshape(-1, 4)
    nm = stats[:, 1].copy() if mean is None else mean
    if mode == "given":
        ns = std
    elif mode == "cdpp":
        ns = np.asarray(cdpp(), dtype=np.float64) * 1e-6
        ns = np.where(np.isnan(ns), stats[:, 2], ns)
    else:
        ns = stats[:, 2].copy()
    return np.ascontiguousarray(nm, dtype=np.float64), np.ascontiguousarray(ns, dtype=np.float64)


def check_stitch(group, B, corrector, order):
    """-> labels int64[B] numbered by first appearance (``group`` None: all zero)."""
    if corrector not in ("normalize", None):
        raise ValueError("corrector must be 'normalize' (the reference's default corrector_func) or None (got %r)" % (corrector,))
    if order not in ("given", "start_time"):
        raise ValueError("order must be 'given' or 'start_time' (got %r)" % (order,))
    if group is None:
        return np.zeros(B, dtype=np.int64)
    g = np.asarray(group)
    if g.ndim != 1 or g.shape[0] != B or g.dtype.kind not in "iub":
        raise ValueError("group must be an integer array with one entry per light curve: shape (%d,), got %s of shape %s"
                         % (B, g.dtype, g.shape))
    first = {}
    return np.array([first.setdefault(int(v), len(first)) for v in g], dtype=np.int64)


def stitch_plan(labels, counts, start_time=None):
    """Which segment goes where: -> (perm int64[B], the segments in output order; seg_off int64[G + 1], the segments of target
    g are perm[seg_off[g]:seg_off[g + 1]]; n_off int64[G + 1], the cadence offsets of the stitched batch).  ``start_time``
    (order="start_time"): the first time of every segment; a target's segments go by it, ties and empty segments in batch
    order, empty ones last."""
    labels = np.asarray(labels, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    B = len(labels)
    G = int(labels.max()) + 1 if B else 1
    if start_time is None:
        perm = np.argsort(labels, kind="stable")
    else:
        key = np.where(counts > 0, np.asarray(start_time, dtype=np.float64), np.inf)
        perm = np.lexsort((np.arange(B), key, labels))
    perm = perm.astype(np.int64)
    seg_off = np.zeros(G + 1, dtype=np.int64)
    seg_off[1:] = np.cumsum(np.bincount(labels, minlength=G))
    dst = np.zeros(B + 1, dtype=np.int64)
    dst[1:] = np.cumsum(counts[perm])
    return perm, seg_off, dst[seg_off]
