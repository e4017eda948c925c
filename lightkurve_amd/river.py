"""River diagrams (cycle x phase images, the data behind ``LightCurve.plot_river`` of lightkurve 2.x): the host side.

Pure numpy, no GPU: the device (``lk_river_plan_batch*``) reports nine numbers per target, and this module turns them and the
caller's arguments into what ``lk_river_batch*`` takes — a status, the number of bins and cycles, the cell offsets and the
edges of every target.  It also holds the numpy mirror of the whole computation (``river_numpy``, what ``LightCurve.river``
returns), which goes through the same layout code.  The role ``foldbin.py`` plays for ``fold_bin``.

The definition (the reference's source is not at hand, so the definition is stated there and is the contract):
``y = flux / nanmedian(flux)``, ``u = flux_err / nanmedian(flux)``; ``n_bins = bins`` or
``int(period / nanmedian(diff(time)) * (maximum_phase - minimum_phase) / bin_points)``; the phase is
``fold(period, epoch_time, normalize_phase=True)``'s, the row ``FoldedLightCurve.cycle``; edges
``np.linspace(minimum_phase, maximum_phase, n_bins + 1)`` and a cadence is in column j when ``edges[j] < phase <= edges[j+1]``
(a phase equal to ``edges[0]`` is in none); a cadence takes part when its y is finite.  ``mean`` / ``median`` of the cell's y, or
``sigma = (mean - 1) / sqrt(nansum(u^2))``; a cell nobody takes part in holds NaN, count 0.

Deviations from the reference, on purpose: rows are this project's cycles (boundary at phase +-0.5 of the given epoch; the reference
cuts at ``time % period``, independent of the epoch); with ``bin_points == 1`` every cell is still aggregated (the reference takes
the cell's first cadence; equal when a cell holds one); ``sigma`` is not divided by the count (the reference's expression).
"""
import numpy as np

NPLAN = 9                        # LK_RIVER_NPLAN (include/lkhip.h)
LDS_CELLS = 3072                 # LK_RIVER_LDS_CELLS: cells per tile (one workgroup); a wider row is cut into column chunks
LDS_VALS = 4096                  # LK_RIVER_LDS_VALS: median, values of a tile collected in LDS (more: device scratch)
CELL_THREAD = 32                 # LK_RIVER_CELL_THREAD: median, values of a cell ranked by one thread (more: the workgroup)
ROUTE_ROWS, ROUTE_COLUMNS, ROUTE_VALS_LDS, ROUTE_VALS_SCRATCH, ROUTE_CELL_THREAD, ROUTE_CELL_GROUP = 1, 2, 4, 8, 16, 32
METHODS = {"mean": 0, "median": 1, "sigma": 2}
STATUS_OK, STATUS_TOO_FEW, STATUS_TIMES, STATUS_SCALE, STATUS_NO_BINS = 0, 1, 2, 3, 4


def check_arguments(B, period, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5, method="mean", bins=None, has_err=True):
    """Validate what ``river`` was given -> (period float64[B], bins int64[B] or None, method code).  ``ValueError`` for a period
    that is not finite and positive, a phase window outside [-0.5, 0.5] or empty, ``bin_points < 1``, ``bins < 1``, an unknown
    method, and ``method="sigma"`` without errors."""
    if method not in METHODS:
        raise ValueError("method must be one of 'mean', 'median', 'sigma' (got %r)" % (method,))
    if method == "sigma" and not has_err:
        raise ValueError("method='sigma' needs flux_err")
    period = np.ascontiguousarray(np.broadcast_to(np.asarray(period, dtype=np.float64), (B,)))
    if not np.all(np.isfinite(period)) or np.any(period <= 0):
        raise ValueError("period must be finite and positive")
    if int(bin_points) != bin_points or bin_points < 1:
        raise ValueError("bin_points must be an integer >= 1")
    minimum_phase, maximum_phase = float(minimum_phase), float(maximum_phase)
    if not (-0.5 <= minimum_phase < maximum_phase <= 0.5):
        raise ValueError("the phase window must satisfy -0.5 <= minimum_phase < maximum_phase <= 0.5")
    if bins is not None:
        bins_f = np.broadcast_to(np.asarray(bins), (B,))
        if np.any(bins_f != np.floor(bins_f)) or np.any(bins_f < 1):
            raise ValueError("bins must be integers >= 1")
        bins = np.ascontiguousarray(bins_f, dtype=np.int64)
    return period, bins, METHODS[method]


def n_bins_of(period, dt, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5):
    """The reference's number of columns: ``int(period / dt * (maximum_phase - minimum_phase) / bin_points)`` in float64, in
    exactly this order."""
    return int(float(period) / float(dt) * (float(maximum_phase) - float(minimum_phase)) / int(bin_points))


def layout(n, plan, period, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5, bins=None, max_output_mb=4096):
    """Statuses and the layout of the output from the device's (or ``plan_numpy``'s) plan.  ``n``: cadences per target; ``plan``:
    float64[B, NPLAN]; ``period`` / ``bins``: as ``check_arguments`` returned them.  Returns dict(status int32[B], n_bins int32[B],
    n_cycles int32[B], cell_off int64[B + 1], edges float64[sum(n_bins) + B] (target b's n_bins + 1 edges at ``edge_off[b]``),
    edge_off int64[B + 1], cycle_min float64[B]).  A target with a non-zero status has no cell.  ``ValueError`` when river and
    count together would exceed ``max_output_mb`` MiB (years of data at a short period make n_cycles x n_bins huge)."""
    n = np.asarray(n, dtype=np.int64)
    B = n.size
    plan = np.asarray(plan, dtype=np.float64).reshape(B, NPLAN)
    med, dt, cmin, cmax, nfin, ok_t = (plan[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        if bins is not None:
            nb = np.asarray(bins, dtype=np.float64)
        else:           # n_bins_of for every target: the same operations in the same order, element by element in float64
            nb = np.trunc(np.asarray(period, dtype=np.float64) / dt * (float(maximum_phase) - float(minimum_phase)) / int(bin_points))
        nb = np.where(np.isfinite(nb), np.minimum(nb, 2.0 ** 62), 0.0)
        status = np.select([(n < 2) | ~(nfin > 0), ~(ok_t > 0), ~np.isfinite(med) | (med == 0.0) | ~(dt > 0), nb < 1],
                           [STATUS_TOO_FEW, STATUS_TIMES, STATUS_SCALE, STATUS_NO_BINS], STATUS_OK).astype(np.int32)
        ok = status == STATUS_OK
        n_bins = np.where(ok, nb, 0.0).astype(np.int64)
        n_cycles = np.where(ok, cmax - cmin + 1.0, 0.0).astype(np.int64)
    cells = (n_bins.astype(object) * n_cycles.astype(object)).tolist()   # (Python integers: no overflow)
    total = sum(cells)
    if total * 12 > float(max_output_mb) * 2 ** 20 or np.any(n_bins >= 2 ** 30) or np.any(n_cycles >= 2 ** 30):
        raise ValueError("the river images need %.1f MiB (%d cells), more than max_output_mb = %g: a longer period, fewer bins or "
                         "fewer targets per call" % (total * 12 / 2.0 ** 20, total, max_output_mb))
    cell_off = np.zeros(B + 1, dtype=np.int64)
    cell_off[1:] = np.cumsum(np.asarray(cells, dtype=np.int64))
    edge_off = np.zeros(B + 1, dtype=np.int64)
    edge_off[1:] = np.cumsum(n_bins + 1)
    edges = np.full(int(edge_off[-1]), np.nan, dtype=np.float64)
    for b in np.flatnonzero(n_bins):
        edges[edge_off[b]:edge_off[b + 1]] = np.linspace(minimum_phase, maximum_phase, int(n_bins[b]) + 1)
    return dict(status=status, n_bins=n_bins.astype(np.int32), n_cycles=n_cycles.astype(np.int32), cell_off=cell_off, edges=edges,
                edge_off=edge_off, cycle_min=np.where(status == 0, plan[:, 2], 0.0))


def split(flat, lay):
    """The packed cells of a batch -> a list of per-target ``(n_cycles_b, n_bins_b)`` arrays (views)."""
    off = lay["cell_off"]
    return [flat[off[b]:off[b + 1]].reshape(int(lay["n_cycles"][b]), int(lay["n_bins"][b])) for b in range(len(off) - 1)]


# ------------------------------------------------------------------------------------------------ numpy mirror
def fold_phase_numpy(time, period, epoch_time):
    """``fold(period, epoch_time, normalize_phase=True)``'s phase in [-0.5, 0.5) with the roundings of ``fold_kernel``:
    ((t - e) + 0 + (P - P/2)) % P - (P - P/2), divided by P."""
    P = np.float64(period)
    shift = P - 0.5 * P
    rel = ((np.asarray(time, dtype=np.float64) - np.float64(epoch_time)) + 0.0 * P) + shift
    return (np.mod(rel, P) - shift) / P


def cycle_numpy(time, period, epoch_time):
    """``FoldedLightCurve.cycle`` before the minimum is taken off: floor((t - (e - P/2)) / P)."""
    P = np.float64(period)
    return np.floor((np.asarray(time, dtype=np.float64) - (np.float64(epoch_time) - P / 2.0)) / P)


def plan_numpy(time, flux, flux_err, period, epoch_time=None):
    """What ``river_plan_kernel`` reports for one light curve -> float64[NPLAN]."""
    t, f = np.asarray(time, dtype=np.float64), np.asarray(flux, dtype=np.float64)
    p = np.zeros(NPLAN, dtype=np.float64)
    t0 = t[0] if t.size else np.nan
    e = t0 if epoch_time is None else float(epoch_time)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            p[0] = np.nanmedian(f) if f.size else np.nan
            d = np.diff(t)
            p[1] = np.nanmedian(d) if d.size else np.nan
        fin_t = np.isfinite(t)
        if fin_t.any():
            c = cycle_numpy(np.array([t[fin_t].min(), t[fin_t].max()]), period, e)
            p[2], p[3] = c.min(), c.max()
        else:
            p[2], p[3] = 0.0, -1.0
        fin = np.isfinite(f)
        p[4] = fin.sum()
        p[5] = 1.0 if fin_t.all() and np.all(d >= 0) else 0.0
        p[6] = t0
        p[7] = np.abs(f[fin]).max() if fin.any() else 0.0
        if flux_err is not None:
            s = np.asarray(flux_err, dtype=np.float64)
            p[8] = np.abs(s[np.isfinite(s)]).max() if np.isfinite(s).any() else 0.0
    return p


def river_numpy(time, flux, flux_err, period, epoch_time=None, bin_points=1, minimum_phase=-0.5, maximum_phase=0.5,
                method="mean", bins=None, max_output_mb=4096):
    """The river image of ONE light curve in numpy (the mirror of the device route) -> dict(river float64[n_cycles, n_bins], count
    int32[n_cycles, n_bins], n_cycles, n_bins, status, edges, cycle_min).  A non-zero status gives empty (0, 0) arrays."""
    t, f = np.asarray(time, dtype=np.float64), np.asarray(flux, dtype=np.float64)
    s = None if flux_err is None else np.asarray(flux_err, dtype=np.float64)
    period, bins, code = check_arguments(1, period, bin_points, minimum_phase, maximum_phase, method, bins, has_err=s is not None)
    plan = plan_numpy(t, f, s, period[0], epoch_time)
    lay = layout([t.size], plan, period, bin_points, minimum_phase, maximum_phase, bins, max_output_mb)
    nb, nc, status = int(lay["n_bins"][0]), int(lay["n_cycles"][0]), int(lay["status"][0])
    edges = lay["edges"][:nb + 1] if status == 0 else np.zeros(0)
    river, count = np.full(nb * nc, np.nan), np.zeros(nb * nc, dtype=np.int32)
    if status == 0:
        e = plan[6] if epoch_time is None else float(epoch_time)
        with np.errstate(all="ignore"):
            y = f / plan[0]
            row = (cycle_numpy(t, period[0], e) - plan[2]).astype(np.int64)
            col = np.searchsorted(edges, fold_phase_numpy(t, period[0], e), side="left") - 1    # edges[j] < phase <= edges[j+1]
            take = (col >= 0) & (col < nb) & np.isfinite(y)
            cell, yt = row[take] * nb + col[take], y[take]
            count[:] = np.bincount(cell, minlength=nb * nc)
            has = count > 0
            if code == METHODS["median"]:
                order = np.lexsort((yt, cell))
                ys, start = yt[order], np.concatenate(([0], np.cumsum(count)[:-1]))
                k = count[has]
                river[has] = (ys[start[has] + (k - 1) // 2] + ys[start[has] + k // 2]) * 0.5
            else:
                river[has] = np.bincount(cell, weights=yt, minlength=nb * nc)[has] / count[has]
                if code == METHODS["sigma"]:
                    u2 = (s[take] / plan[0]) ** 2
                    s2 = np.bincount(cell, weights=np.where(np.isnan(u2), 0.0, u2), minlength=nb * nc)
                    river[has] = (river[has] - 1.0) / np.sqrt(s2[has])
    return dict(river=river.reshape(nc, nb), count=count.reshape(nc, nb), n_cycles=nc, n_bins=nb, status=status, edges=edges,
                cycle_min=float(lay["cycle_min"][0]))
