"""Inputs of the resident seismology tests (test_device_seismology_cpu.py / _gpu.py): two grids of 3000 frequencies and
five synthetic oscillation spectra, and the reference's deltanu planning written with its own expressions; and, further
down, the integer-valued windows and the case table of test_seismology_exact_gpu.py, with a numpy-only reference."""
import zlib

import numpy as np

from lightkurve_amd import seismology

M = 3000
GRIDS = {"rg": np.arange(50, 3050) * 0.1, "ms": np.arange(300, 3300) * 1.0}      # microhertz
TRUE_NUMAX = {"rg": (60.0, 120.0, 200.0), "ms": (1200.0, 2000.0)}


def spectrum(grid, numax, i):
    """Envelope of Lorentzian modes (radial, an l=2 neighbour, the l=1 ridge half way) times chi^2_2 noise, seed 100 + i."""
    f, ms = GRIDS[grid], grid == "ms"
    fs = f[1] - f[0]
    rng = np.random.default_rng(100 + i)
    dnu = 0.294 * numax ** 0.772
    fwhm = 0.25 * numax if ms else 0.66 * numax ** 0.88
    env = np.exp(-0.5 * ((f - numax) / (fwhm / 2.355)) ** 2)
    width = max(2 * fs, 0.02 * dnu)
    modes = np.zeros(M)
    for n in range(-12, 13):
        for off, h in ((0.0, 1.0), (-0.13 * dnu, 0.6), (0.5 * dnu, 0.8)):
            modes += h / (1 + ((f - (numax + n * dnu + off)) / width) ** 2)
    return (1 + 25 * env * modes) * rng.exponential(size=M)


def batch(grid):
    """(frequency, power[B, M], true numax[B]); spectrum k of a grid has seed 100 + k."""
    nm = TRUE_NUMAX[grid]
    return GRIDS[grid], np.stack([spectrum(grid, v, k) for k, v in enumerate(nm)]), np.array(nm)


def reference_deltanu_plan(frequency, numax):
    """What estimate_deltanu_acf2d derives from numax, by its own lines (seismology.py, deltanu_estimators.py:95-126): the
    window, the distance and the selection as the full mask over np.linspace.  Frequencies in microhertz."""
    fs = np.median(np.diff(frequency))
    deltanu_emp = 0.294 * numax ** 0.772
    fwhm = 0.25 * numax if frequency[-1] > 500.0 else 0.66 * numax ** 0.88
    window_width = 2 * int(np.floor(fwhm))
    start, W = seismology._window_start(frequency, numax, window_width, fs)
    lags = np.linspace(0.0, W * fs, W)
    sel = (lags > deltanu_emp - 0.25 * deltanu_emp) & (lags < deltanu_emp + 0.25 * deltanu_emp)
    return dict(start=start, width=W, deltanu_emp=deltanu_emp, distance=np.floor(deltanu_emp / 2.0 / fs), lags=lags, sel=sel)


# ------------------------------------------------------------------------------------------------ exact deltanu cases
# Windows on which rounding decides nothing (test_seismology_exact_gpu.py, guarded on numpy alone by
# test_device_seismology_cpu.py): p[0] = A = -sum(h), p[sel_lo + j] = h[j] (positive integers), zero elsewhere.  The sum is
# exactly 0, so nanmean is 0 in any order of addition; the selection (0.75 emp, 1.25 emp) / step has n <= sel_lo, so two
# samples of h are never a selected lag apart and C[sel_lo + j] = A h[j] exactly; the rescaled ACF is the same three
# correctly rounded operations for everyone and strictly monotone in h.  The order structure of the slice is that of h.
M_EXACT = 20000
LDS_DOUBLES = 160 * 1024 // 8          # the launcher's stated limit: W + 16 + n doubles


def lags_of(W, step, stop):
    lags = np.arange(W) * step
    lags[-1] = stop
    return lags


def selection(W, emp, step, stop):
    """(sel_lo, n) of the two-sided strict selection; one run in every case of this file (asserted)."""
    lags = lags_of(W, step, stop)
    idx = np.flatnonzero((lags > emp - 0.25 * emp) & (lags < emp + 0.25 * emp))
    if idx.size == 0:
        return 0, 0
    assert idx[-1] - idx[0] + 1 == idx.size
    return int(idx[0]), int(idx.size)


def exact_window(W, sel_lo, h):
    h = np.asarray(h, dtype=np.int64)
    assert 1 <= h.size <= sel_lo and sel_lo + h.size <= W and h.min() >= 1
    p = np.zeros(W)
    p[sel_lo:sel_lo + h.size] = h
    p[0] = -h.sum()
    return p


def reference_acf(p_window, emp, step, stop):
    """numpy alone: (C, rescaled acf, sel_lo, n) of one window; lines of deltanu_estimators.py / utils.py."""
    p = np.asarray(p_window, dtype=np.float64)
    W = p.size
    with np.errstate(all="ignore"):
        q = p - np.nanmean(p)
        C = np.correlate(q, q, "full")[W - 1:]
        acf = (np.abs(C ** 2) / np.abs(C[0] ** 2)) / (3 / (2 * len(C)))
    return (C, acf) + selection(W, emp, step, stop)


def find_peaks_stable(x, distance):
    """scipy.signal.find_peaks(x, distance=) with the priorities ordered by a STABLE argsort: of equally high peaks the later
    one is served first.  scipy's own argsort is unstable in general and agrees with this on short peak lists."""
    x = np.asarray(x, dtype=np.float64)
    peaks = seismology._local_maxima_1d(x)
    keep = np.ones(len(peaks), dtype=bool)
    dist = int(np.ceil(distance))
    order = np.argsort(x[peaks], kind="stable")
    for j in order[::-1]:
        if keep[j]:
            keep &= ~(np.abs(peaks - peaks[j]) < dist)
            keep[j] = True
    return peaks[keep]


def reference_deltanu_from_tables(p_window, emp, distance, step, stop, find_peaks=seismology._find_peaks):
    """The reference on one window and one row of the six tables -> dict, or None where it would raise (fewer than 3 selected
    lags, distance < 1 or NaN, no peak)."""
    C, acf, lo, n = reference_acf(p_window, emp, step, stop)
    if n < 3 or not distance >= 1:
        return None
    x = acf[lo:lo + n]
    peaks = find_peaks(x, distance)
    if len(peaks) == 0:
        return None
    lags = lags_of(len(C), step, stop)[lo:lo + n]
    k = int(np.argmin(np.abs(lags[peaks] - emp)))
    return dict(deltanu=float(lags[peaks][k]), winner=int(peaks[k]), peaks=peaks, maxima=seismology._local_maxima_1d(x),
                x=x, lags=lags, sel_lo=lo, sel_len=n)


def _spikes(n, pos, heights, base=1):
    h = np.full(n, base, dtype=np.int64)
    h[np.asarray(pos)] = heights
    return h


def _peaky(n, seed, gaps=(2, 3, 4)):
    """Maxima every 2 to 4 samples from slice index 1 on, all heights distinct (2 ..)."""
    rng = np.random.default_rng(seed)
    pos, i = [], 1
    while i <= n - 2:
        pos.append(i)
        i += int(rng.choice(gaps))
    return _spikes(n, pos, 2 + rng.permutation(len(pos)))


def _sparse(n, seed, count):
    """`count` maxima of distinct heights at odd slice indices spread over the whole slice."""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(np.arange(1, n - 1, 2), size=count, replace=False))
    return _spikes(n, pos, 2 + rng.permutation(count))


def _plateaus(n):
    h = np.full(n, 5, dtype=np.int64)
    h[0:3] = 50                      # touches the start of the slice: no peak
    h[n - 3:n] = 51                  # touches its end: no peak
    h[10:12] = 20                    # width 2 -> 10
    h[20:23] = 21                    # width 3 -> 21
    h[40:45] = 23                    # width 5 -> 42
    h[62:66] = 24                    # width 4 over lanes 63 | 64 -> 63
    h[100:103], h[103] = 26, 30      # a plateau followed by a rise: 103 alone
    h[147:151] = 22                  # width 4 next to emp (slice index 149) -> 148
    h[254:258] = 25                  # width 4 over threads 255 | 256 -> 255
    return h


def emp_for_sel_len(W, n, lo=8000.0, hi=8400.0):
    """The first emp on a grid of 0.5 (step 1, stop W - 1) whose selection has exactly n lags."""
    for emp in np.arange(lo, hi, 0.5):
        if selection(W, float(emp), 1.0, W - 1.0)[1] == n:
            return float(emp)
    raise ValueError("no emp selects %d lags" % n)


def _case(name, W, emp, distance, h=None, window=None, step=1.0, stop=None, start=100, status=0, maxima=0, survivors=0,
          winner=-1, tie=False, group="exact", plan_sel_len=None):
    stop = (W - 1) * step if stop is None else stop
    lo, n = selection(W, emp, step, stop) if 2 <= W <= 16384 else (0, 0)
    if callable(h):
        h = h(n)
    if h is not None:
        h = np.asarray(h, dtype=np.int64)
        window = exact_window(W, lo, h)
    return dict(name=name, W=W, start=start, emp=emp, distance=distance, step=step, stop=stop, h=h, window=window,
                status=status, maxima=maxima, survivors=survivors, winner=winner, tie=tie, group=group, sel_lo=lo, sel_len=n,
                plan_sel_len=n if plan_sel_len is None else plan_sel_len)


def _production(name, grid, numax, h, **kw):
    """The tables seismology._deltanu_plan gives this numax on a grid of this file (stop = W fs, step = stop / (W - 1))."""
    pl = reference_deltanu_plan(GRIDS[grid], numax)
    return _case(name, pl["width"], pl["deltanu_emp"], pl["distance"], h, step=pl["lags"][1], stop=pl["lags"][-1], **kw)


PRODUCTION_NUMAX = {"rg": 120.0, "ms": 2005.0}
_TWO = dict(pos=[30, 60, 76, 110], heights=[900, 500, 400, 800])        # emp = 300, step 1: n = 149, emp at slice index 74
_E4080 = emp_for_sel_len(16384, LDS_DOUBLES - 16384 - 16)
_E4081 = emp_for_sel_len(16384, LDS_DOUBLES - 16384 - 16 + 1)


def _two(n):
    return _spikes(n, **_TWO)


def _build_cases():
    c = []
    # two survivors.  At the production ratio distance = floor(emp / 2 / step) the slice is shorter than the distance (n - 3 <
    # ceil(distance): two maxima that both survive do not fit), so the two-survivor cases halve it: floor(emp / 4 / step).
    c.append(_case("two_survivors_nearer_later", 800, 300.0, 75.0, _two, start=123, maxima=4, survivors=2, winner=110))
    c.append(_case("two_survivors_nearer_earlier", 800, 300.0, 75.0, lambda n: _spikes(n, [40, 72, 90, 120], [800, 300, 350, 900]),
                   start=1001, maxima=4, survivors=2, winner=40))
    c.append(_case("production_ratio_one_survivor", 800, 300.0, 150.0, _two, start=7, maxima=4, survivors=1, winner=30))
    # 2 d = ceil(distance) exactly: the two are just far enough apart to both survive
    c.append(_case("equidistant_tie", 800, 300.0, 75.5, lambda n: _spikes(n, [36, 112], [700, 900]), start=3000, maxima=2,
                   survivors=2, winner=36, tie=True))
    c.append(_production("production_lags_rg", "rg", PRODUCTION_NUMAX["rg"], lambda n: _spikes(n, [n // 2 - 9, n // 2 + 5], [40, 90]),
                         start=5000, maxima=2, survivors=1, winner=34))
    c.append(_production("production_lags_ms", "ms", PRODUCTION_NUMAX["ms"], lambda n: _spikes(n, [3, n // 2 + 2, n - 4], [7, 60, 9]),
                         start=6001, maxima=3, survivors=1, winner=28))
    c.append(_case("plateaus", 800, 600.0, 1.0, _plateaus, start=9000, maxima=7, survivors=7, winner=148))
    c.append(_case("plateaus_distance", 800, 600.0, 43.0, _plateaus, start=9600, maxima=7, survivors=4, winner=148))
    # (maxima, then per distance: survivors, winner) as the reference gave them once; test_device_seismology_cpu.py holds them
    many = (("n299", 800, 600.0, 11, 96, ((1.0, 96, 149), (4.2, 40, 146), (40.0, 7, 139), (309.0, 1, 268), (3e9, 1, 268))),
            ("n999", 4096, 2000.0, 12, 327, ((1.0, 327, 499), (4.2, 134, 503), (40.0, 19, 503), (1009.0, 1, 37), (3e9, 1, 37))))
    for n_name, W, emp, seed, maxima, rows in many:
        for d_name, (dist, survivors, winner) in zip(("1", "4p2", "40", "n_plus_10", "3e9"), rows):
            c.append(_case("many_%s_distance_%s" % (n_name, d_name), W, emp, dist, lambda n, seed=seed: _peaky(n, seed),
                           start=2000 + len(c), maxima=maxima, survivors=survivors, winner=winner))
    c.append(_case("maxima_at_slice_edges", 800, 300.0, 75.0, lambda n: _spikes(n, [1, n - 2], [50, 60]), start=40, maxima=2,
                   survivors=2, winner=1, tie=True))
    c.append(_case("selection_to_last_lag", 375, 300.0, 75.0, lambda n: _spikes(n, [100, n - 2], [60, 70]), stop=374.5, start=15000,
                   maxima=2, survivors=1, winner=147))
    c.append(_case("n3_middle_highest", 16, 6.0, 1.0, [1, 5, 2], start=19000, maxima=1, survivors=1, winner=1))
    # status 3
    c.append(_case("monotone", 800, 300.0, 75.0, lambda n: np.arange(1, n + 1), start=300, status=3))
    c.append(_case("n2", 16, 4.4, 1.0, [3, 2], start=19100, status=3))
    for d_name, dist in (("half", 0.5), ("zero", 0.0), ("nan", np.nan)):
        c.append(_case("distance_" + d_name, 800, 300.0, dist, _two, start=400 + len(c), status=3))
    c.append(_case("constant_window", 400, 100.0, 20.0, window=np.full(400, 7.0), start=11000, status=3, group="raw"))
    nan_window = exact_window(800, 226, _two(149))
    nan_window[5] = np.nan
    c.append(_case("one_nan", 800, 300.0, 75.0, window=nan_window, start=12000, status=3, group="raw"))
    # largest window
    c.append(_case("w16384_n99", 16384, 200.0, 25.0, lambda n: _spikes(n, [10, 45, 52, 80], [30, 50, 45, 20]), start=3616, maxima=4,
                   survivors=3, winner=45))
    c.append(_case("w16384_lds_exactly_full", 16384, _E4080, 40.0, lambda n: _sparse(n, 13, 100), start=0, maxima=100, survivors=49,
                   winner=2043))
    # equal heights (the documented rule: the later of equally high peaks is served first)
    c.append(_case("equal_two", 800, 300.0, 75.0, lambda n: _spikes(n, [60, 90], [500, 500]), start=13000, maxima=2, survivors=1,
                   winner=90, group="equal"))
    c.append(_case("equal_three", 800, 300.0, 25.0, lambda n: _spikes(n, [50, 70, 100], [500, 500, 500]), start=14000, maxima=3,
                   survivors=2, winner=70, group="equal"))
    # status 2
    c.append(_case("start_minus_1", 800, 300.0, 75.0, start=-1, status=2, group="refused"))
    c.append(_case("ends_past_the_row", 800, 300.0, 75.0, start=M_EXACT + 1 - 800, status=2, group="refused"))
    c.append(_case("w1", 1, 300.0, 75.0, start=50, status=2, group="refused"))
    c.append(_case("w16385", 16385, 200.0, 25.0, start=10, status=2, group="refused"))
    c.append(_case("understated_sel_len_alone", 400, 300.0, 75.0, _two, start=16000, status=2, group="refused", plan_sel_len=10))
    c.append(_case("w16384_lds_one_lag_too_many", 16384, _E4081, 40.0, lambda n: _sparse(n, 14, 100), start=1, status=2, group="refused"))
    return c


CASES = _build_cases()
CASE = {c["name"]: c for c in CASES}
RUN_CASES = [c for c in CASES if c["group"] != "refused"]          # status 0 or 3: one batch
REFUSED_CASES = [c for c in CASES if c["group"] == "refused"]      # status 2
# truncated output: the understated target beside a wider one whose LDS suffices for both (max_sel = 10 < 149)
TRUNCATED_PAIR = [_case("understated_sel_len", 400, 300.0, 75.0, _two, start=16000, maxima=4, survivors=2, winner=110, plan_sel_len=10),
                  _case("wider_neighbour", 800, 16.0, 2.0, [1, 4, 1, 1, 6, 2, 1], start=17000, maxima=2, survivors=2, winner=4)]


def case_row(c, M=M_EXACT, start=None):
    """The spectrum row of a case: its window at `start` in M other integers (1 .. 9, seeded by the case's name)."""
    row = np.random.default_rng(zlib.crc32(c["name"].encode())).integers(1, 10, M).astype(np.float64)
    c = dict(c, start=c["start"] if start is None else start)
    if c["window"] is not None and c["start"] >= 0 and c["start"] + c["W"] <= M:
        row[c["start"]:c["start"] + c["W"]] = c["window"]
    return row


def case_plan(cs):
    """The dict _capi.pg_deltanu_batch takes, written by hand from the cases (seismology._deltanu_plan is not involved)."""
    return dict(start=np.array([c["start"] for c in cs], dtype=np.int32), width=np.array([c["W"] for c in cs], dtype=np.int32),
                deltanu_emp=np.array([c["emp"] for c in cs]), distance=np.array([c["distance"] for c in cs]),
                step=np.array([c["step"] for c in cs]), stop=np.array([c["stop"] for c in cs]),
                sel_len=np.array([c["plan_sel_len"] for c in cs], dtype=np.int32))


_REFERENCE = {}


def case_reference(c):
    """(reference dict or None, acf row on the selection or None), computed once per case and shared read-only."""
    if c["name"] not in _REFERENCE:
        if c["window"] is None or c["group"] == "refused" and c["name"] != "understated_sel_len_alone":
            _REFERENCE[c["name"]] = (None, None)
        else:
            fp = find_peaks_stable if c["group"] == "equal" else seismology._find_peaks
            _, acf, lo, n = reference_acf(c["window"], c["emp"], c["step"], c["stop"])
            _REFERENCE[c["name"]] = (reference_deltanu_from_tables(c["window"], c["emp"], c["distance"], c["step"], c["stop"], fp),
                                     acf[lo:lo + n])
    return _REFERENCE[c["name"]]
