"""GPU: the seismology kernels of csrc/pgsmooth.hip (pg_deltanu_kernel, pg_acf2d_kernel and its two helpers, pg_numax_pick_kernel,
pg_divide_kernel) on inputs where rounding decides nothing, against numpy and seismology._find_peaks (pinned to scipy by
test_seismology_gpu.py and test_device_seismology_cpu.py), never against the entry points themselves.

deltanu: the case table of seismology_cases.py (integer-valued zero-sum windows: C[sel] = A h exactly, the slice ordered as
the integer array h; every claim of the table is proven on numpy alone in test_device_seismology_cpu.py).  The hand-written
plans go straight into _capi.pg_deltanu_batch: all cases in one batch, each alone, the refused ones mixed in.  status,
sel_lo, sel_len, n_peaks, deltanu and the acf slice are compared with ==.
2-D ACF: integer-valued zero-sum windows of 1 .. 16384 samples, acf2d and metric with ==.
numax pick: ties, NaN and -inf rows with ==; the Gaussian-smoothed metric within 1e-12 relative, argmax identical.
SNR division: == numpy, both kernels, with guard words around the output.

The only tolerances are taken over from test_device_seismology_gpu.py / test_seismology_gpu.py:
  smoothed metric, 1e-12 relative (np.correlate's order of addition is not the kernel's): measured maximum 1.9e-15
  (n_win = 1000, 253 taps; 2.8e-16 at n_win = 11);
  the two float-valued ACF windows, 1e-12 of the zero lag (BLAS ddot order): measured maxima 9.6e-16 (W = 1027) and
  1.0e-14 (W = 16384); their metric, 1e-12 relative: 3.7e-16 and 2.0e-16.
The tests print what they measure (pytest -s)."""
import ctypes
import functools

import numpy as np
import pytest

import seismology_cases as cases
from lightkurve_amd import _capi, seismology
from lightkurve_amd.device import DeviceBuffer, DevicePeriodogramBatch

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
LDS_REFUSED = ("understated_sel_len_alone", "w16384_lds_one_lag_too_many")     # status 2 after the selection was counted
KEYS = ("deltanu", "n_peaks", "status", "sel_lo", "sel_len")


# ------------------------------------------------------------------------------------------------ deltanu
def run(cs):
    power = np.stack([cases.case_row(c) for c in cs])
    return _capi.pg_deltanu_batch(power, cases.case_plan(cs), want_acf=True)


@functools.lru_cache(maxsize=None)
def run_all():
    return run(cases.RUN_CASES)


def check(out, b, c):
    """Row b of a result against the numpy reference of case c, everything with ==."""
    ref, x = cases.case_reference(c)
    lo, n = c["sel_lo"], c["sel_len"]
    row = out["acf"][b]
    assert out["status"][b] == c["status"], c["name"]
    if c["status"] == 0:
        assert ref is not None and (out["sel_lo"][b], out["sel_len"][b]) == (lo, n) == (ref["sel_lo"], ref["sel_len"]), c["name"]
        assert out["n_peaks"][b] == len(ref["peaks"]) == c["survivors"], c["name"]
        assert out["deltanu"][b] == ref["deltanu"], c["name"]
    else:
        assert ref is None or c["name"] in LDS_REFUSED
        assert np.isnan(out["deltanu"][b]) and out["n_peaks"][b] == 0, c["name"]
        want_sel = (lo, n) if c["status"] == 3 or c["name"] in LDS_REFUSED else (0, 0)
        assert (out["sel_lo"][b], out["sel_len"][b]) == want_sel, c["name"]
    m = min(n, row.size)
    if c["status"] == 2 or n < 3 or not c["distance"] >= 1:
        assert np.isnan(row).all(), c["name"]                       # nothing was formed
    else:
        assert np.array_equal(row[:m], x[:m], equal_nan=True), c["name"]
        assert np.isnan(row[n:]).all(), c["name"]


def test_every_case_in_one_batch():
    out = run_all()
    assert out["acf"].shape == (len(cases.RUN_CASES), cases.LDS_DOUBLES - 16384 - 16)
    for b, c in enumerate(cases.RUN_CASES):
        check(out, b, c)
    assert sorted(set(out["status"].tolist())) == [0, 3]


@pytest.mark.parametrize("c", cases.RUN_CASES, ids=lambda c: c["name"])
def test_case_alone_equals_reference_and_batch(c):
    one, many, b = run([c]), run_all(), cases.RUN_CASES.index(c)
    check(one, 0, c)
    for key in KEYS:
        assert np.array_equal(one[key][0], many[key][b], equal_nan=True), key
    n = c["sel_len"]
    assert one["acf"].shape[1] == n and np.array_equal(one["acf"][0], many["acf"][b, :n], equal_nan=True)


@pytest.mark.parametrize("c", cases.REFUSED_CASES, ids=lambda c: c["name"])
def test_refused_case_alone(c):
    check(run([c]), 0, c)


def test_refused_cases_leave_their_neighbours_alone():
    """Status-2 targets between the others: the others' outputs keep their bits."""
    refused = [c for c in cases.REFUSED_CASES if c["name"] != "understated_sel_len_alone"]      # (beside wide targets it fits)
    mixed, where = [], {}
    for k, c in enumerate(cases.RUN_CASES):
        if k % 7 == 0 and k // 7 < len(refused):
            mixed.append(refused[k // 7])
        where[c["name"]] = len(mixed)
        mixed.append(c)
    assert all(r in mixed for r in refused)
    out, base = run(mixed), run_all()
    w = base["acf"].shape[1]
    for b, c in enumerate(mixed):
        if c["group"] == "refused":
            check(out, b, c)
    for k, c in enumerate(cases.RUN_CASES):
        b = where[c["name"]]
        for key in KEYS:
            assert np.array_equal(out[key][b], base[key][k], equal_nan=True), (c["name"], key)
        assert np.array_equal(out["acf"][b, :w], base["acf"][k], equal_nan=True) and np.isnan(out["acf"][b, w:]).all(), c["name"]


def test_truncated_acf_row():
    """A plan whose sel_len understates a target's selection: beside a wider target the LDS suffices, the result is right and
    the acf row holds the first max_sel values."""
    short, wide = cases.TRUNCATED_PAIR
    out = run([short, wide])
    assert out["acf"].shape == (2, 10)
    check(out, 0, short)
    check(out, 1, wide)
    assert not np.isnan(out["acf"][0]).any() and np.isnan(out["acf"][1, wide["sel_len"]:]).all()


@pytest.mark.parametrize("grid", ["rg", "ms"])
def test_resident_path_on_a_planned_exact_window(grid):
    """DevicePeriodogramBatch.estimate_deltanu with the production planner: the exact window sits where the planner puts the
    window of this numax.  (Two surviving peaks cannot occur at the planner's distance: test_device_seismology_cpu.py.)"""
    f, numax, c = cases.GRIDS[grid], cases.PRODUCTION_NUMAX[grid], cases.CASE["production_lags_" + grid]
    pl = cases.reference_deltanu_plan(f, numax)
    ref, x = cases.case_reference(c)
    rows = np.stack([cases.case_row(c, cases.M, pl["start"]), cases.case_row(dict(c, name=c["name"] + "/2"), cases.M, pl["start"])])
    dn = DevicePeriodogramBatch.from_arrays(f, rows).estimate_deltanu(numax, return_acf=True)
    alone = run([c])
    for b in range(2):
        assert dn["status"][b] == 0 and dn["deltanu"][b] == ref["deltanu"] == alone["deltanu"][0]
        assert dn["n_peaks"][b] == len(ref["peaks"]) and dn["deltanu_emp"][b] == pl["deltanu_emp"]
        assert (dn["sel_lo"][b], dn["sel_len"][b]) == (c["sel_lo"], c["sel_len"])
        assert np.array_equal(dn["acf"][b], x) and np.array_equal(dn["acf"][b], alone["acf"][0])


# ------------------------------------------------------------------------------------------------ 2-D ACF
ACF_W = (1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2050, 16384)


def np_acf(win):
    W = win.size
    with np.errstate(all="ignore"):
        q = win - np.nanmean(win)
        C = np.correlate(q, q, mode="full")[W - 1:]
        return C, (np.sum(np.abs(C)) - 1) / W


def acf_rows(W, seed, integer=True, nan_at=None):
    """B = 2 rows with three windows of W samples at starts of different alignment; integer: values in -8 .. 8 with the last
    (non-NaN) sample set so that the window sums to zero."""
    rng = np.random.default_rng(seed)
    starts = np.array([0, W + 3, 2 * W + 10], dtype=np.int32)
    M = 3 * W + 10
    rows = rng.integers(-8, 9, (2, M)).astype(np.float64) if integer else rng.exponential(size=(2, M))
    for b in range(2):
        for k, s in enumerate(starts):
            win = rows[b, s:s + W]
            last = W - 1
            if nan_at is not None:
                win[nan_at[k]] = np.nan
                last = W - 2 if nan_at[k] == W - 1 else W - 1
            if integer:
                win[last] -= np.nansum(win)
                assert np.nansum(win) == 0
    return rows, starts


def acf_metric_only(power, starts, W):
    """lk_pg_acf_metric_batch_dev on device buffers."""
    h = _capi.Handle.get(0)
    B, M = power.shape
    d_pow, d_met = DeviceBuffer(h, power.nbytes), DeviceBuffer(h, B * starts.size * 8)
    keep = d_pow.upload(power)
    _capi._check(_capi._lib.lk_pg_acf_metric_batch_dev(h._h, B, M, _vp(d_pow.ptr), int(starts.size), starts.ctypes.data_as(_i32p), W,
                                                       _vp(d_met.ptr), None))
    out = d_met.download(np.float64, B * starts.size).reshape(B, starts.size)
    del keep
    return out


@pytest.mark.parametrize("W", ACF_W)
def test_acf2d_of_integer_windows_is_exact(W):
    """Every product and partial sum is an integer below 2^53: acf2d and metric == numpy in any order of addition."""
    rows, starts = acf_rows(W, 1000 + W)
    acf, met = _capi.pg_acf2d_batch(rows, starts, W)
    assert acf.shape == (2, 3, W)
    for b in range(2):
        for k, s in enumerate(starts):
            C, metric = np_acf(rows[b, s:s + W])
            assert np.sum(np.abs(C)) < 2.0 ** 53 and np.array_equal(C, np.round(C))
            assert np.array_equal(acf[b, k], C), (b, k)
            assert met[b, k] == metric, (b, k)
    assert np.array_equal(acf_metric_only(rows, starts, W), met)


def test_acf2d_refuses_more_than_16384_samples():
    rows = np.ones((1, 16385))
    with pytest.raises(ValueError, match="outside 1..16384"):
        _capi.pg_acf2d_batch(rows, [0], 16385)


@pytest.mark.parametrize("W", (5, 257, 1025))
def test_acf2d_nan_pattern_is_numpys(W):
    """One NaN per window, at its first, middle and last sample: the lags numpy leaves finite are finite and equal."""
    rows, starts = acf_rows(W, 2000 + W, nan_at=(0, W // 2, W - 1))
    acf, met = _capi.pg_acf2d_batch(rows, starts, W)
    finite = 0
    for b in range(2):
        for k, s in enumerate(starts):
            C, metric = np_acf(rows[b, s:s + W])
            assert np.array_equal(np.isnan(acf[b, k]), np.isnan(C)) and np.array_equal(acf[b, k], C, equal_nan=True), (b, k)
            assert np.isnan(metric) and np.isnan(met[b, k])
            finite += int(np.sum(~np.isnan(C)))
    assert finite == 2 * (W - 1 - W // 2)                     # the middle NaN spares the lags it is not paired at
    assert np.isnan(acf_metric_only(rows, starts, W)).all()


@pytest.mark.parametrize("W", (1027, 16384))
def test_acf2d_of_float_windows(W):
    """Ordinary data on the odd and the long path, at the tolerance of test_seismology_gpu.py: 1e-12 of the zero lag."""
    rows, starts = acf_rows(W, 3000 + W, integer=False)
    acf, met = _capi.pg_acf2d_batch(rows, starts, W)
    worst = worst_met = 0.0
    for b in range(2):
        for k, s in enumerate(starts):
            C, metric = np_acf(rows[b, s:s + W])
            worst = max(worst, float(np.max(np.abs(acf[b, k] - C)) / C[0]))
            worst_met = max(worst_met, abs(met[b, k] - metric) / abs(metric))
    print("acf2d W = %d: max |acf - numpy| / zero lag = %.3e, metric relative %.3e" % (W, worst, worst_met))
    assert worst < 1e-12 and worst_met < 1e-12
    assert np.array_equal(acf_metric_only(rows, starts, W), met)


# ------------------------------------------------------------------------------------------------ numax pick
def numax_pick(metric, taps=None, alias=False):
    """lk_pg_numax_pick_batch_dev on device buffers -> (metric as left on the device, metric_smooth, argmax)."""
    h = _capi.Handle.get(0)
    metric = np.ascontiguousarray(np.atleast_2d(metric), dtype=np.float64)
    B, n_win = metric.shape
    d_met = DeviceBuffer(h, metric.nbytes)
    d_smooth = d_met if alias else DeviceBuffer(h, metric.nbytes)
    d_arg = DeviceBuffer(h, B * 8)
    keep = d_met.upload(metric)
    taps = None if taps is None else np.ascontiguousarray(taps, dtype=np.float64)
    _capi._check(_capi._lib.lk_pg_numax_pick_batch_dev(h._h, B, n_win, _vp(d_met.ptr), None if taps is None else taps.ctypes.data_as(_dp),
                                                       0 if taps is None else int(taps.size), _vp(d_smooth.ptr), _vp(d_arg.ptr), None))
    arg = d_arg.download(np.int64, B)
    del keep
    return (d_met.download(np.float64, B * n_win).reshape(B, n_win), d_smooth.download(np.float64, B * n_win).reshape(B, n_win), arg)


@functools.lru_cache(maxsize=None)
def smooth_rows(n_win):
    """Three metric-like rows (a bump on noise) and their reference, with the guard that rounding cannot decide the argmax."""
    rng = np.random.default_rng(4000 + n_win)
    i = np.arange(n_win)
    rows = np.stack([1.0 + 4.0 * np.exp(-0.5 * ((i - c * n_win) / (0.08 * n_win + 1.0)) ** 2) + 0.3 * rng.random(n_win)
                     for c in (0.03, 0.5, 0.97)])                      # maxima at both clamped edges and in the middle
    ref = np.stack([seismology._gaussian_smooth_extend(r, np.sqrt(n_win)) for r in rows])
    for r in ref:
        top = np.sort(r)[-2:]
        assert top[1] - top[0] > 1e-6 * top[1]
    return rows, ref


@pytest.mark.parametrize("n_win", (11, 12, 27, 255, 256, 257, 1000))
def test_numax_pick_with_taps(n_win):
    rows, ref = smooth_rows(n_win)
    taps = seismology._gaussian_taps(np.sqrt(n_win))
    if n_win == 11:
        assert taps.size == 27                                          # more taps than windows: both clamps at once
    left, smooth, arg = numax_pick(rows, taps)
    worst = float(np.max(np.abs(smooth - ref) / np.abs(ref)))
    print("numax pick n_win = %d, %d taps: max relative error of the smoothed metric %.3e" % (n_win, taps.size, worst))
    assert np.array_equal(left, rows)
    assert np.allclose(smooth, ref, rtol=1e-12, atol=0)
    assert np.array_equal(arg, np.argmax(ref, axis=1))


def tie_rows(n_win):
    """Integer metrics with equal maxima (value 9 over 0 .. 5): (row, expected argmax) pairs for this n_win."""
    rng = np.random.default_rng(5000 + n_win)
    out = []

    def row(at, value=9.0, fill=None):
        r = rng.integers(0, 6, n_win).astype(np.float64) if fill is None else np.full(n_win, fill)
        for k in at:
            if k < n_win:
                r[k] = value
        return r

    if n_win >= 300:
        out.append((row([261, 5] if n_win < 518 else [261, 517, 773]), 5 if n_win < 518 else 261))      # one lane's stride
        out.append((row([299, 45]), 45))                                 # lanes 43 and 45 of wave 0, the later lane first
        out.append((row([200, 130, 290]), 130))                          # waves 3, 2 and 0 (second trip)
        out.append((row([64, 128, 192]), 64))                            # lane 0 of waves 1, 2, 3
        nan_row = row([3], np.inf)
        nan_row[[270, 90]] = np.nan
        out.append((nan_row, 90))                                        # a NaN beats +inf, the first NaN wins
        out.append((row([n_win - 1]), n_win - 1))
    if n_win == 2:
        out += [(np.array([3.0, 3.0]), 0), (np.array([1.0, np.nan]), 1), (np.array([np.inf, np.nan]), 1), (np.array([2.0, 5.0]), 1)]
    if n_win == 1:
        out += [(np.array([7.0]), 0), (np.array([-7.0]), 0)]
    out.append((np.full(n_win, np.nan), 0))
    out.append((np.full(n_win, -np.inf), 0))
    out.append((np.full(n_win, 4.0), 0))
    return np.stack([r for r, _ in out]), np.array([k for _, k in out])


@pytest.mark.parametrize("alias", (False, True), ids=("separate", "aliased"))
@pytest.mark.parametrize("n_win", (1, 2, 300, 1000))
def test_numax_pick_without_taps_takes_the_first_maximum(n_win, alias):
    rows, want = tie_rows(n_win)
    for r, k in zip(rows, want):
        assert np.argmax(r) == k                                         # the expectation is numpy's
    left, smooth, arg = numax_pick(rows, None, alias)
    assert np.array_equal(arg, want)
    assert np.array_equal(left, rows, equal_nan=True) and np.array_equal(smooth, rows, equal_nan=True)


# ------------------------------------------------------------------------------------------------ SNR division
@pytest.mark.parametrize("offset", (0, 16, 8), ids=("aligned", "aligned_plus_16", "plus_8"))
def test_snr_division_is_numpys(offset):
    """B M = 3003 is odd: the 16-byte kernel ends in a single element.  8 bytes into larger buffers no pointer is 16-byte
    aligned and the scalar kernel runs.  The words around the output keep their bits."""
    B, M = 3, 1001
    n, pad = B * M, offset // 8
    rng = np.random.default_rng(6000 + offset)
    power, bkg = rng.exponential(size=n), rng.exponential(size=n) + 0.5
    power[[0, 7, 500, n - 1]] = [0.0, 3.0, np.nan, 0.0]
    bkg[[0, 7, 501, n - 1, n - 2]] = [0.0, 0.0, np.nan, 0.0, -0.0]
    power[n - 2] = 2.0                                                   # 2 / -0 = -inf
    with np.errstate(all="ignore"):
        want = power / bkg
    assert np.isnan(want[[0, 500, 501, n - 1]]).all() and want[7] == np.inf and want[n - 2] == -np.inf
    h = _capi.Handle.get(0)
    guard = -12345.678
    host = [np.concatenate([np.full(pad, guard), a, np.full(1, guard)]) for a in (power, bkg, np.full(n, guard))]
    bufs = [DeviceBuffer(h, a.nbytes) for a in host]
    keep = [b.upload(a) for b, a in zip(bufs, host)]
    assert all(b.ptr % 16 == 0 for b in bufs)
    _capi._check(_capi._lib.lk_pg_snr_batch_dev(h._h, B, M, _vp(bufs[0].ptr + offset), _vp(bufs[1].ptr + offset),
                                                _vp(bufs[2].ptr + offset), None))
    got = bufs[2].download(np.float64, n + pad + 1)
    del keep
    assert np.array_equal(got[pad:pad + n], want, equal_nan=True)
    ok = ~np.isnan(want)
    assert np.array_equal(np.signbit(got[pad:pad + n][ok]), np.signbit(want[ok]))
    assert np.all(got[:pad] == guard) and got[pad + n] == guard
