"""Inputs of the river-diagram tests and an independent restatement of the definition.

Imports nothing from the package.  ``reference`` is a double loop over the cells of the image with boolean masks; its phase and
cycle are written differently from the package's (``((t - e) / P + 0.5) % 1 - 0.5`` and ``floor((t - e) / P + 0.5)``), which is
the same number up to rounding.  So that rounding never decides a membership, every case is built with no cadence within MARGIN
(in phase) of a bin edge or of the cycle boundary, and ``reference`` asserts that for every case it is given — the exception is the
dyadic case (``exact=True``), where every quantity is an exact binary fraction, and a cadence at the epoch itself, whose phase is
exactly 0 in any formulation.  With that no cell is ever left out of a comparison.
"""
import functools

import numpy as np

MARGIN = 1e-9
LENGTHS = (5000, 1, 63, 0, 64, 65, 1500, 2)
PERIODS = (3.7, 1.0, 5.0, 1.0, 1.0, 0.31, 2.3, 0.5)        # many cycles, -, one, -, two, five, fourteen, one
LDS_CELLS, LDS_VALS, CELL_THREAD = 3072, 4096, 32            # include/lkhip.h's LK_RIVER_* (test_river_cpu checks the mirror)


def light_curve(n, seed, period, cadence=0.0204, t0=1325.0, scale=870.0, nan_every=0):
    """A jittered, strictly increasing light curve with a 1 % transit at phase 0 of ``period`` and positive errors."""
    rng = np.random.RandomState(seed)
    t = t0 + cadence * np.arange(n) + cadence * 0.2 * rng.rand(n)
    f = 1.0 + 2e-3 * rng.randn(n)
    if n:
        f[np.abs(((t - t[0]) / period + 0.5) % 1.0 - 0.5) < 0.04] -= 0.01
    f *= scale
    s = scale * 2e-3 * (1.0 + 0.3 * rng.rand(n))
    if nan_every:
        f[::nan_every] = np.nan
    return dict(time=t, flux=f, flux_err=s, period=float(period), epoch=None)


@functools.lru_cache(maxsize=None)
def ragged():
    return tuple(light_curve(n, 100 + i, P, nan_every=(97 if n >= 1000 else 0)) for i, (n, P) in enumerate(zip(LENGTHS, PERIODS)))


def dyadic(n=64):
    """Every quantity an exact binary fraction: phases fall ON edges, and one cadence per cycle sits at phase -0.5."""
    return dict(time=np.arange(n) / 8.0, flux=np.arange(n) + 1.0, flux_err=np.full(n, 0.5), period=1.0, epoch=0.0)


def gap():
    """600 cadences with a hole of 3.5 periods in the middle: rows without a cadence."""
    lc = light_curve(600, 7, 1.3)
    lc["time"][300:] += 3.5 * 1.3
    return lc


def bad_values():
    """NaN and +-inf flux, NaN errors (so that some cells have no finite error at all)."""
    lc = light_curve(800, 11, 1.9)
    lc["flux"][5::37] = np.nan
    lc["flux"][100], lc["flux"][333], lc["flux"][500] = np.inf, -np.inf, np.inf
    lc["flux_err"][3::11] = np.nan
    lc["flux_err"][200:260] = np.nan
    return lc


def window_batch():
    return tuple(light_curve(n, 40 + i, P) for i, (n, P) in enumerate(((900, 2.1), (700, 0.77), (1200, 4.4))))


def large_cells():
    """bin_points = 300 on 6000 cadences: six columns, cells of about 330 cadences."""
    return light_curve(6000, 21, 40.0, cadence=0.02)


def one_row(n, seed, duplicates=False):
    """n cadences inside ONE cycle, none at phase -0.5; with duplicates a quarter of the times repeat an earlier one (fewer than
    half of the differences are zero, so the median step stays positive)."""
    lc = light_curve(n, seed, 1.0, cadence=0.001)
    if duplicates:
        base = lc["time"][:n - n // 4]
        lc["time"] = np.sort(np.concatenate([base, base[::2][:n // 4]]))
        assert lc["time"].size == n and np.nanmedian(np.diff(lc["time"])) > 0
    span = lc["time"][-1] - lc["time"][0]
    lc["period"], lc["epoch"] = 4.3 * max(span, 1.0), float(lc["time"][0] + 0.37 * span)
    return lc


def route_targets():
    """A target on each side of every route threshold; each entry: (name, light curve, bins)."""
    wide = light_curve(4000, 61, 50.0)                          # 81.6 d at P = 50: rows 0..2
    return (("cells_at", wide, LDS_CELLS), ("cells_over", wide, LDS_CELLS + 1),
            ("vals_at", one_row(LDS_VALS, 62), 8), ("vals_over", one_row(LDS_VALS + 1, 63), 8),
            ("vals_dup", one_row(LDS_VALS + 104, 64, duplicates=True), 8),
            ("cell_at", one_row(CELL_THREAD, 65), 1), ("cell_over", one_row(CELL_THREAD + 1, 66), 1))


def status_batch():
    """(light curve, expected status): one target per non-zero status in the middle of good ones."""
    good = [light_curve(300 + 17 * i, 80 + i, 1.1 + 0.3 * i) for i in range(5)]
    one = light_curve(1, 90, 1.0)
    unsorted = light_curve(200, 91, 1.0)
    unsorted["time"][[50, 51]] = unsorted["time"][[51, 50]]
    zero_med = light_curve(200, 92, 1.0)
    zero_med["flux"][:150] = 0.0
    no_bins = light_curve(50, 93, 0.01)                         # period below the cadence: int(P / dt) == 0
    return ((good[0], 0), (one, 1), (good[1], 0), (unsorted, 2), (good[2], 0), (zero_med, 3), (good[3], 0), (no_bins, 4),
            (good[4], 0))


def expected_status(lc, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5, bins=None):
    t, f = lc["time"], lc["flux"]
    if t.size < 2 or not np.isfinite(f).any():
        return 1
    if not np.all(np.isfinite(t)) or np.any(np.diff(t) < 0):
        return 2
    med, dt = np.nanmedian(f), np.nanmedian(np.diff(t))
    if not np.isfinite(med) or med == 0 or not dt > 0:
        return 3
    nb = bins if bins is not None else int(lc["period"] / dt * (maximum_phase - minimum_phase) / bin_points)
    return 4 if nb < 1 else 0


def reference(lc, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5, method="mean", bins=None, exact=False):
    """The definition, cell by cell -> dict(status, n_cycles, n_bins, river, count, edges)."""
    t, f, s, P = lc["time"], lc["flux"], lc["flux_err"], lc["period"]
    status = expected_status(lc, bin_points, minimum_phase, maximum_phase, bins)
    if status:
        return dict(status=status, n_cycles=0, n_bins=0, river=np.zeros((0, 0)), count=np.zeros((0, 0), dtype=np.int32),
                    edges=np.zeros(0))
    e = t[0] if lc["epoch"] is None else lc["epoch"]
    med, dt = np.nanmedian(f), np.nanmedian(np.diff(t))
    nb = bins if bins is not None else int(P / dt * (maximum_phase - minimum_phase) / bin_points)
    with np.errstate(all="ignore"):
        y = f / med
        u = s / med if s is not None else None
    x = (t - e) / P + 0.5
    phase, cycle = x % 1.0 - 0.5, np.floor(x).astype(np.int64)
    cycle -= cycle.min()
    nc = int(cycle.max()) + 1
    edges = np.linspace(minimum_phase, maximum_phase, nb + 1)
    if not exact:
        bounds = np.unique(np.concatenate([edges, [-0.5, 0.5]]))
        at = np.searchsorted(bounds, phase)
        dist = np.minimum(np.abs(phase - bounds[np.clip(at, 0, bounds.size - 1)]),
                          np.abs(phase - bounds[np.clip(at - 1, 0, bounds.size - 1)]))
        # (a cadence AT the epoch — the first one, where no epoch is given — has phase exactly 0 however it is written)
        dist = dist[t != e].min() if np.any(t != e) else 1.0
        assert dist > MARGIN, "a cadence lies within %g of a bin edge or the cycle boundary (%g)" % (MARGIN, dist)
    river, count = np.full((nc, nb), np.nan), np.zeros((nc, nb), dtype=np.int32)
    fin = np.isfinite(y)
    with np.errstate(all="ignore"):
        for r in range(nc):
            rows = np.flatnonzero(cycle == r)
            ph, yr, fr = phase[rows], y[rows], fin[rows]
            for j in range(nb):
                m = (ph > edges[j]) & (ph <= edges[j + 1]) & fr
                k = int(m.sum())
                count[r, j] = k
                if k == 0:
                    continue
                if method == "mean":
                    river[r, j] = np.mean(yr[m])
                elif method == "median":
                    river[r, j] = np.median(yr[m])
                else:
                    river[r, j] = (np.mean(yr[m]) - 1.0) / np.sqrt(np.nansum(u[rows][m] ** 2))
    return dict(status=0, n_cycles=nc, n_bins=nb, river=river, count=count, edges=edges)


def compare(got, ref, method, label=""):
    """One target's image against the restatement: shape, counts and the NaN / inf pattern equal; the median equal with no
    tolerance; mean and sigma within the house rule 1e-9 max(1, |ref|).  ``got``: dict(river, count, status, n_cycles, n_bins).
    Returns the largest |difference| / max(1, |ref|) over the finite cells (printed before it is asserted)."""
    assert int(got["status"]) == ref["status"], (label, got["status"], ref["status"])
    assert (int(got["n_cycles"]), int(got["n_bins"])) == (ref["n_cycles"], ref["n_bins"]), label
    r, c = np.asarray(got["river"]), np.asarray(got["count"])
    assert r.shape == ref["river"].shape and c.shape == ref["count"].shape and c.dtype == np.int32 and r.dtype == np.float64, label
    assert np.array_equal(c, ref["count"]), label
    assert np.array_equal(np.isnan(r), np.isnan(ref["river"])) and np.array_equal(c == 0, np.isnan(r) & (c == 0)), label
    if method == "median":
        assert np.array_equal(r, ref["river"], equal_nan=True), label
        return 0.0
    fin = np.isfinite(ref["river"])
    assert np.array_equal(r[~fin], ref["river"][~fin], equal_nan=True), label          # +-inf of sigma's zero denominator
    worst = float(np.max(np.abs(r[fin] - ref["river"][fin]) / np.maximum(1.0, np.abs(ref["river"][fin])))) if fin.any() else 0.0
    print("%s %s: max |d| / max(1, |ref|) = %.3g over %d cells" % (label, method, worst, int(fin.sum())))
    assert worst <= 1e-9, (label, worst)
    return worst


def pack(lcs, with_err=True):
    """-> time, flux, flux_err, n_off, period, epoch (None when no light curve names one; where only some do, the others get
    their first time, which is what the default means)."""
    n_off = np.concatenate([[0], np.cumsum([lc["time"].size for lc in lcs])]).astype(np.int64)
    cat = lambda k: np.concatenate([lc[k] for lc in lcs]) if lcs else np.zeros(0)
    first = lambda lc: float(lc["time"][0]) if lc["time"].size else 0.0
    epoch = None if all(lc["epoch"] is None for lc in lcs) else np.array([first(lc) if lc["epoch"] is None else lc["epoch"]
                                                                          for lc in lcs])
    return cat("time"), cat("flux"), (cat("flux_err") if with_err else None), n_off, np.array([lc["period"] for lc in lcs]), epoch
