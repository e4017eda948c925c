"""The numpy restatement of ``LightCurve.fill_gaps`` (lightkurve 2.x, method="gaussian_noise") on both of its paths, and the
batch of light curves test_fillgaps_cpu.py, test_fillgaps_gpu.py and test_stitch_gpu.py share (no test in here).

The restatement is written with elementary expressions, every product and sum its own numpy operation, so that no library's
contraction decides a bit; the time path's loop is a literal transcription of the reference's.  It marks the inserted cadences
by construction and leaves their flux out: the reference draws it from numpy's global generator, the device from its Philox
stream (``overfit_cases.normals``).

The batch, by cadence count after the gaps and the NaN-flux cadences are cut (``LENGTHS``):
  0      empty
  1      a single cadence (fewer than 2: unchanged)
  2      two cadences (one step: nothing to insert)
  63     one single missing cadence
  64     no gap at all: the output equals the input
  65     three adjacent missing cadences; the flux_err of the original before them is NaN
  1500   a gap directly after the first original and one directly before the last; on the time path also a step of 1.1875 m
         (inserts nothing) and one of 1.25 m (inserts exactly one cadence)
  5000   one gap of 3000 cadences and 40 scattered NaN fluxes (those cadences become gaps); on the cadence path its cadence
         numbers start at 1 200 000
Time path: times ``2 + k / 64`` (binary fractions: every threshold decision and every link of a chain is exact, m = 1 / 64, and
refilling what was cut reproduces the full grid bit for bit).  Cadence path: barycentric-like jittered times
``m0 c (1 + 1e-6 sin(c / 900)) + 1e-7 noise`` that increase with the cadence number (asserted)."""
import functools

import numpy as np

LENGTHS = (0, 1, 2, 63, 64, 65, 1500, 5000)
QUALITY_INSERTED = 65536
M0 = 1.0 / 64.0                       # time path: the grid step
M0_CAD = 0.02043229                   # cadence path: a TESS-like 30-minute step [d]
SHIFT_NONE, SHIFT_ONE = 0.1875, 0.25  # time path, light curve 6: extra steps in units of m (1.1875 m: nothing; 1.25 m: one)
SHIFT_AT = (600, 900)                 # ... in front of these grid cadences
FIRST_CADENCE = (0, 10, 20, 300, 4000, 5000, 70000, 1200000)


def _cuts(b):
    """-> (grid cadences K, sorted array of the grid indices that are cut, grid indices whose flux is NaN)."""
    n = LENGTHS[b]
    none = np.zeros(0, dtype=np.int64)
    if b in (0, 1, 2, 4):
        return n, none, none
    if b == 3:
        return 64, np.array([10]), none
    if b == 5:
        return 68, np.array([20, 21, 22]), none
    if b == 6:
        K = 1500 + 2 + 5
        return K, np.array([1, 700, 701, 1000, 1001, 1002, K - 2]), none
    K = 5000 + 3000 + 40
    nan = np.arange(40) * 97 + 4100          # behind the long gap, never adjacent to each other
    return K, np.arange(1000, 4000), nan


@functools.lru_cache(maxsize=None)
def batch(path):
    """The light curves as the caller hands them over (NaN fluxes still in) -> tuple of dicts(time, flux, flux_err, quality,
    cadenceno); read-only arrays."""
    out = []
    for b, n in enumerate(LENGTHS):
        K, cut, nan = _cuts(b)
        rng = np.random.default_rng(100 + b)
        k = np.setdiff1d(np.arange(K), cut)
        c = (FIRST_CADENCE[b] + k).astype(np.int32)
        if path == "time":
            t = 2.0 + k / 64.0
            if b == 6:
                t = t + np.where(k >= SHIFT_AT[0], SHIFT_NONE * M0, 0.0) + np.where(k >= SHIFT_AT[1], SHIFT_ONE * M0, 0.0)
        else:
            cf = c.astype(np.float64)
            t = M0_CAD * cf * (1.0 + 1e-6 * np.sin(cf / 900.0)) + 1e-7 * rng.standard_normal(k.size)
            assert np.all(np.diff(t) > 0), "cadence-path times must increase with the cadence number"
        flux = 1.0 + 0.01 * rng.standard_normal(k.size)
        flux[np.isin(k, nan)] = np.nan
        err = 0.01 * (1.0 + 0.1 * rng.random(k.size))
        if b == 5:
            err[19] = np.nan                # the original in front of the three missing cadences
        q = (rng.integers(0, 4, k.size) * 128).astype(np.int32)
        assert int(np.sum(~np.isnan(flux))) == n
        lc = dict(time=t, flux=flux, flux_err=err, quality=q, cadenceno=c)
        for a in lc.values():
            a.setflags(write=False)
        out.append(lc)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the restatement
def _interp(x, j, xp, fp):
    """np.interp's expression between points j and j + 1: slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]), slope (x - xp[j]) + fp[j],
    every operation rounded on its own (no NaN repair: a NaN end gives NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
        return slope * (x - xp[j]) + fp[j]


def time_path_times(time):
    """The reference's loop, literally -> (ntime, inserted bool)."""
    dt = np.median(np.diff(time))
    ntime, ins = [time[0]], [False]
    for t in time[1:]:
        prevtime = ntime[-1]
        while (t - prevtime) > 1.2 * dt:
            ntime.append(prevtime + dt)
            ins.append(True)
            prevtime = ntime[-1]
        ntime.append(t)
        ins.append(False)
    return np.asarray(ntime, float), np.asarray(ins, bool)


def cadence_path_times(time, cadenceno):
    """-> (ntime, ncad int32, inserted bool): every cadence number of [c_first, c_last]; d = t - m cf per original, linear in cf
    inside a gap (np.interp's expression), plus m cf — for the originals too, as the reference recomputes them."""
    m = np.median(np.diff(time))
    cf = cadenceno.astype(np.float64)
    d = time - m * cf
    ncad = np.arange(int(cadenceno[0]), int(cadenceno[-1]) + 1, dtype=np.int64)
    ins = np.ones(ncad.size, dtype=bool)
    ins[cadenceno.astype(np.int64) - int(cadenceno[0])] = False
    ncf = ncad.astype(np.float64)
    nd = np.empty(ncad.size)
    nd[~ins] = d
    j = np.searchsorted(cadenceno, ncad[ins], side="right") - 1
    nd[ins] = _interp(ncf[ins], j, cf, d)
    return nd + m * ncf, ncad.astype(np.int32), ins


def fill_gaps(lc, path, with_err=True, with_quality=True):
    """The filled light curve without the flux of its inserted cadences -> dict(time, flux (NaN where inserted), flux_err,
    quality, cadenceno, inserted, m, mu, sd, n_inserted, original: the light curve after remove_nans)."""
    keep = ~np.isnan(lc["flux"])
    t, f, e, q, c = (lc[k][keep] for k in ("time", "flux", "flux_err", "quality", "cadenceno"))
    orig = dict(time=t, flux=f, flux_err=e if with_err else None, quality=q if with_quality else None,
                cadenceno=c if path == "cadenceno" else None)
    n = t.size
    mu = np.nanmean(f) if n else np.nan
    sd = np.nanstd(f) if n else np.nan
    if n < 2:
        return dict(orig, inserted=np.zeros(n, dtype=bool), m=np.nan, mu=mu, sd=sd, n_inserted=0, original=orig)
    m = np.median(np.diff(t))
    if path == "time":
        nt, ins = time_path_times(t)
        nc = None
    else:
        nt, nc, ins = cadence_path_times(t, c)
    nf = np.full(nt.size, np.nan)
    nf[~ins] = f
    ne = nq = None
    j = np.cumsum(~ins)[ins] - 1                 # the original in front of every inserted cadence
    if with_err:
        ne = np.empty(nt.size)
        ne[~ins] = e
        ne[ins] = _interp(nt[ins], j, t, e)      # against the ORIGINAL times, as the reference's np.interp(ntime, lc.time, ...)
    if with_quality:
        nq = np.full(nt.size, QUALITY_INSERTED, dtype=np.int32)
        nq[~ins] = q
    return dict(time=nt, flux=nf, flux_err=ne, quality=nq, cadenceno=nc, inserted=ins, m=m, mu=mu, sd=sd,
                n_inserted=int(ins.sum()), original=orig)


@functools.lru_cache(maxsize=None)
def expected(path, with_err=True, with_quality=True):
    """``fill_gaps`` of every light curve of ``batch(path)``; cached, shared by the tests, read-only."""
    out = tuple(fill_gaps(lc, path, with_err, with_quality) for lc in batch(path))
    for r in out:
        for a in list(r.values()) + list(r["original"].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def pack(lcs, keys=("time", "flux", "flux_err", "quality", "cadenceno")):
    """A list of dicts -> (dict of concatenated columns (None where a light curve has None), n_off)."""
    n_off = np.concatenate([[0], np.cumsum([lc["time"].size for lc in lcs])]).astype(np.int64)
    cols = {}
    for k in keys:
        if any(lc.get(k) is None for lc in lcs):
            cols[k] = None
        else:
            cols[k] = np.concatenate([lc[k] for lc in lcs]) if lcs else np.zeros(0, dtype=np.float64)
    return cols, n_off
