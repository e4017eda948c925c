"""GPU: the resident seismology chain (device.DevicePeriodogramBatch: flatten -> estimate_numax -> estimate_deltanu, and
seismology.estimate_deltanu_acf2d_batch) against a numpy restatement of the reference kept in this file:
np.correlate(sel - nanmean(sel), ..., "full")[W - 1:], (sum |C| - 1) / W, and the host helpers
seismology._gaussian_smooth_extend / _find_peaks (pinned by goldens and scipy in test_seismology_gpu.py) — never the new
entry points themselves.

Tolerances (stated): metric and smoothed metric 1e-12 relative (np.correlate sums through BLAS ddot, whose order is not
the kernel's); the rescaled ACF on the selection rtol 1e-10, atol 1e-12 of its maximum (test_seismology_gpu.py's bound);
numax, the selection, n_peaks and deltanu identical.  Before any comparison the inputs are checked on the reference alone:
its numax within 10 % of the truth, the two largest smoothed-metric values more than 1e-6 apart (relative), the winning
ACF peak more than 1e-6 above both neighbours — so "identical" is asked only where rounding cannot decide.

CPU figures of the reference on seismology_cases' spectra (numax found / window samples / deltanu found): rg 62.5 / 500 /
6.81, 118.5 / 880 / 12.01, 189.5 / 1320 / 17.61; ms 1195 / 596 / 69.12, 2005 / 1002 / 104.10; n_win 274 (rg) and 275 (ms),
W = 250; 35-84 lags selected, one peak survives."""
import functools

import numpy as np
import pytest

import seismology_cases as cases
from lightkurve_amd import _capi, seismology
from lightkurve_amd.device import DeviceLightCurveBatch, DevicePeriodogramBatch
from lightkurve_amd.periodogram import Periodogram

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ numpy reference
def ref_numax(f, p, numaxs=None):
    numaxs, _, starts, W = seismology._plan(Periodogram(f, p, frequency_unit="uHz"), numaxs, None, None)
    metric = np.empty(len(starts))
    for k, s in enumerate(starts):
        sel = p[s:s + W].copy()
        sel -= np.nanmean(sel)
        C = np.correlate(sel, sel, mode="full")[W - 1:]
        metric[k] = (np.sum(np.abs(C)) - 1) / W
    smooth = seismology._gaussian_smooth_extend(metric, np.sqrt(len(numaxs))) if len(numaxs) > 10 else metric
    return dict(numaxs=numaxs, metric=metric, metric_smooth=smooth, arg=int(np.argmax(smooth)),
                numax=float(numaxs[np.argmax(smooth)]))


def ref_deltanu(f, p, numax):
    pl = cases.reference_deltanu_plan(f, numax)
    sel_p = p[pl["start"]:pl["start"] + pl["width"]].copy()
    sel_p -= np.nanmean(sel_p)
    C = np.correlate(sel_p, sel_p, mode="full")[len(sel_p) - 1:]
    acf = (np.abs(C ** 2) / np.abs(C[0] ** 2)) / (3 / (2 * len(C)))
    lags, sel = pl["lags"], pl["sel"]
    peaks = seismology._find_peaks(acf[sel], distance=pl["distance"])
    best = lags[sel][peaks][np.argmin(np.abs(lags[sel][peaks] - pl["deltanu_emp"]))]
    return dict(deltanu=float(best), acf=acf, sel=sel, peaks=peaks, deltanu_emp=pl["deltanu_emp"], lags=lags)


@functools.lru_cache(maxsize=None)
def reference(grid):
    """The reference on the grid's batch, run once and shared (read-only), with the guards on the inputs."""
    f, power, truth = cases.batch(grid)
    out = []
    for p, true_numax in zip(power, truth):
        nm = ref_numax(f, p)
        assert abs(nm["numax"] - true_numax) < 0.1 * true_numax
        top = np.sort(nm["metric_smooth"])[-2:]
        assert top[1] - top[0] > 1e-6 * top[1]
        dn = ref_deltanu(f, p, nm["numax"])
        x = dn["acf"][dn["sel"]]
        k = dn["peaks"][np.argmin(np.abs(dn["lags"][dn["sel"]][dn["peaks"]] - dn["deltanu_emp"]))]
        assert x[k] - max(x[k - 1], x[k + 1]) > 1e-6 * x[k]
        out.append((nm, dn))
    return f, power, out


@functools.lru_cache(maxsize=None)
def device(grid):
    f, power, _ = cases.batch(grid)
    pgs = DevicePeriodogramBatch.from_arrays(f, power)
    nm = pgs.estimate_numax(return_metric=True)
    dn = pgs.estimate_deltanu(return_acf=True)
    return pgs, nm, dn


def check_acf_slice(got_row, lo, n, ref):
    idx = np.flatnonzero(ref["sel"])
    assert (lo, n) == (idx[0], idx.size) and idx[-1] - idx[0] + 1 == n
    want = ref["acf"][idx]
    assert np.allclose(got_row[:n], want, rtol=1e-10, atol=1e-12 * np.max(want))
    assert np.isnan(got_row[n:]).all()


# ------------------------------------------------------------------------------------------------ numax and deltanu
@pytest.mark.parametrize("grid", ["rg", "ms"])
def test_numax_and_deltanu_vs_numpy(grid):
    f, power, ref = reference(grid)
    pgs, nm, dn = device(grid)
    assert nm["metric"].shape == (len(power), 274 if grid == "rg" else 275)
    for b, (rn, rd) in enumerate(ref):
        assert np.array_equal(nm["numaxs"], rn["numaxs"])
        assert np.allclose(nm["metric"][b], rn["metric"], rtol=1e-12, atol=0)
        assert np.allclose(nm["metric_smooth"][b], rn["metric_smooth"], rtol=1e-12, atol=0)
        assert nm["numax"][b] == rn["numax"]
        check_acf_slice(dn["acf"][b], dn["sel_lo"][b], dn["sel_len"][b], rd)
        assert dn["n_peaks"][b] == len(rd["peaks"]) and dn["deltanu"][b] == rd["deltanu"]
        assert dn["deltanu_emp"][b] == rd["deltanu_emp"]
    assert (dn["status"] == 0).all()


@pytest.mark.parametrize("grid", ["rg", "ms"])
def test_metric_only_kernel_is_the_acf2d_metric(grid):
    """lk_pg_acf_metric_batch_dev == the metric of lk_pg_acf2d_batch, bit for bit."""
    f, power, _ = cases.batch(grid)
    _, _, starts, W = seismology._plan(Periodogram(f, power[0], frequency_unit="uHz"), None, None, None)
    _, met = _capi.pg_acf2d_batch(power, starts, W)
    assert np.array_equal(device(grid)[1]["metric"], met)


def test_nan_sample_follows_numpy():
    """A NaN in the spectrum poisons the windows that hold it; np.argmax takes the first NaN of the smoothed metric, and the
    deltanu window around that numax is clean."""
    f, power, _ = cases.batch("rg")
    p = power[0].copy()
    p[cases.M // 2] = np.nan
    rn = ref_numax(f, p)
    assert np.isnan(rn["metric_smooth"]).any() and rn["arg"] == int(np.flatnonzero(np.isnan(rn["metric_smooth"]))[0])
    rd = ref_deltanu(f, p, rn["numax"])
    pgs = DevicePeriodogramBatch.from_arrays(f, p)
    nm = pgs.estimate_numax(return_metric=True)
    for key in ("metric", "metric_smooth"):
        assert np.array_equal(np.isnan(nm[key][0]), np.isnan(rn[key]))
        ok = ~np.isnan(rn[key])
        assert np.allclose(nm[key][0][ok], rn[key][ok], rtol=1e-12, atol=0)
    assert nm["numax"][0] == rn["numax"]
    dn = pgs.estimate_deltanu(return_acf=True)
    check_acf_slice(dn["acf"][0], dn["sel_lo"][0], dn["sel_len"][0], rd)
    assert dn["status"][0] == 0 and dn["deltanu"][0] == rd["deltanu"] and dn["n_peaks"][0] == len(rd["peaks"])


def test_custom_numaxs_are_not_smoothed():
    f, power, _ = cases.batch("rg")
    numaxs = np.linspace(40.0, 250.0, 8)
    nm = DevicePeriodogramBatch.from_arrays(f, power).estimate_numax(numaxs=numaxs, return_metric=True)
    assert np.array_equal(nm["metric"], nm["metric_smooth"])
    for b, p in enumerate(power):
        rn = ref_numax(f, p, numaxs)
        top = np.sort(rn["metric"])[-2:]
        assert top[1] - top[0] > 1e-6 * top[1]
        assert np.allclose(nm["metric"][b], rn["metric"], rtol=1e-12, atol=0) and nm["numax"][b] == rn["numax"]


def test_deltanu_statuses_leave_neighbours_alone():
    f, power, ref = reference("rg")
    good = [rn["numax"] for rn, _ in ref]
    pgs = DevicePeriodogramBatch.from_arrays(f, np.concatenate([power, power[:2]]))
    dn = pgs.estimate_deltanu(numax=good + [np.nan, f[-1] - 1.0])
    assert dn["status"].tolist() == [0, 0, 0, 1, 2]
    assert np.isnan(dn["deltanu"][3:]).all() and (dn["n_peaks"][3:] == 0).all()
    assert np.array_equal(dn["deltanu"][:3], device("rg")[2]["deltanu"])
    assert np.array_equal(pgs.estimate_deltanu(numax=-1.0)["status"], np.full(5, 1))
    with pytest.raises(ValueError):
        DevicePeriodogramBatch.from_arrays(f, power).estimate_deltanu()          # no numax yet


def test_alone_in_batch_and_twice_bitwise():
    f, power, _ = cases.batch("ms")
    _, nm, dn = device("ms")
    one = DevicePeriodogramBatch.from_arrays(f, power[1])
    nm1 = one.estimate_numax(return_metric=True)
    dn1 = one.estimate_deltanu(return_acf=True)
    for key in ("metric", "metric_smooth", "numax"):
        assert np.array_equal(nm1[key][0], nm[key][1])
    n = dn["sel_len"][1]
    assert dn1["sel_len"][0] == n and np.array_equal(dn1["acf"][0][:n], dn["acf"][1][:n])
    assert dn1["deltanu"][0] == dn["deltanu"][1]
    again = DevicePeriodogramBatch.from_arrays(f, power)
    nm2 = again.estimate_numax(return_metric=True)
    dn2 = again.estimate_deltanu(return_acf=True)
    for key in ("metric", "metric_smooth", "numax"):
        assert np.array_equal(nm2[key], nm[key])
    for key in ("deltanu", "n_peaks", "status", "sel_lo", "sel_len", "acf"):
        assert np.array_equal(dn2[key], dn[key], equal_nan=True)


# ------------------------------------------------------------------------------------------------ smooth / flatten / chain
def test_flatten_and_smooth_equal_the_host_class():
    f, power, _ = cases.batch("rg")
    pgs = DevicePeriodogramBatch.from_arrays(f, power)
    snr, bkg = pgs.flatten(method="logmedian", filter_width=0.01, return_trend=True)
    box = pgs.smooth("boxkernel", filter_width=2.0).to_host()
    got_snr, got_bkg = snr.to_host(), bkg.to_host()
    assert snr.power_unit == "" and [type(x) for x in snr.to_periodograms()] == [Periodogram] * 3
    for b, p in enumerate(power):
        host = Periodogram(f, p, frequency_unit="uHz")
        h_snr, h_bkg = host.flatten(method="logmedian", filter_width=0.01, return_trend=True)
        assert np.array_equal(got_snr[b], h_snr.power) and np.array_equal(got_bkg[b], h_bkg.power)
        assert np.array_equal(box[b], host.smooth("boxkernel", filter_width=2.0).power)
    pk = pgs.peaks()
    assert np.array_equal(pk["argmax"], np.argmax(power, axis=1)) and np.array_equal(pk["max_power"], power.max(axis=1))
    assert np.array_equal(pk["frequency"], f[np.argmax(power, axis=1)])
    with pytest.raises(ValueError, match="must be larger than 0"):
        pgs.smooth("boxkernel", filter_width=0.0)
    with pytest.raises(ValueError, match="not supported"):
        pgs.smooth("median")


def test_chain_from_light_curves_equals_the_steps():
    """batch.to_periodogram(f, 'psd').estimate_seismology() == the same kernels called step by step through the host."""
    rng = np.random.default_rng(5)
    t = np.arange(2000) * (2.0 / 1440.0)
    f = np.arange(300, 3300) * 1.0
    time, flux = [], []
    for k in range(4):
        numax = 1000.0 + 300.0 * k
        y = 1.0 + 1e-4 * rng.normal(size=t.size)
        for n in range(-4, 5):
            y += 2e-4 * np.exp(-0.5 * (n / 2.5) ** 2) * np.sin(2 * np.pi * (numax + n * 0.294 * numax ** 0.772) * 1e-6 * 86400.0 * t
                                                                 + rng.uniform(0, 6.28))
        time.append(t + 0.01 * k)
        flux.append(y)
    n_off = np.arange(5) * t.size
    lcs = DeviceLightCurveBatch.from_arrays(np.concatenate(time), np.concatenate(flux), None, n_off)
    pgs = lcs.to_periodogram(f, normalization="psd")
    assert pgs.frequency_unit == "uHz" and len(pgs) == 4
    res = pgs.estimate_seismology()
    host_power = lcs.to_periodogram_power(f, normalization="psd", to_host=True)
    assert np.array_equal(pgs.to_host(), host_power)
    steps = DevicePeriodogramBatch.from_arrays(f, host_power)
    snr = steps.flatten()
    numax = snr.estimate_numax()["numax"]
    dn = snr.estimate_deltanu()
    assert np.array_equal(res["numax"], numax) and np.array_equal(res["deltanu"], dn["deltanu"], equal_nan=True)
    assert np.array_equal(res["status"], dn["status"]) and np.array_equal(pgs.numax, numax)


def test_deltanu_batch_equals_single_calls():
    """seismology.estimate_deltanu_acf2d_batch (lk_pg_deltanu_batch) against estimate_deltanu_acf2d per target."""
    for grid in ("rg", "ms"):
        f, power, ref = reference(grid)
        pgl = [Periodogram(f, p, frequency_unit="uHz") for p in power]
        numaxs = [rn["numax"] for rn, _ in ref]
        many = seismology.estimate_deltanu_acf2d_batch(pgl, numaxs)
        for pg, nm, got in zip(pgl, numaxs, many):
            one = seismology.estimate_deltanu_acf2d(pg, nm)
            assert got["status"] == 0 and got["deltanu"] == one["deltanu"] and got["deltanu_emp"] == one["deltanu_emp"]
            assert np.array_equal(got["peaks"], one["peaks"]) and np.array_equal(got["sel"], one["sel"])
            assert got["n_peaks"] == len(one["peaks"]) and np.array_equal(got["lags"], one["lags"])
            s = one["sel"]
            assert np.allclose(got["acf"][s], one["acf"][s], rtol=1e-10, atol=1e-12 * np.max(one["acf"][s]))
            assert np.isnan(got["acf"][~s]).all()
    assert seismology.estimate_deltanu_acf2d_batch([], []) == []
    with pytest.raises(ValueError, match="one shared frequency grid"):
        seismology.estimate_deltanu_acf2d_batch([pgl[0], Periodogram(f + 1.0, power[0], frequency_unit="uHz")], 1000.0)


def test_plan_errors_are_the_host_ones():
    f, power, _ = cases.batch("rg")
    uneven = f.copy()
    uneven[10] += 0.03
    with pytest.raises(ValueError, match="uniformly spaced"):
        DevicePeriodogramBatch.from_arrays(uneven, power).estimate_numax()
    with pytest.raises(ValueError, match="uniformly spaced"):
        DevicePeriodogramBatch.from_arrays(uneven, power).estimate_deltanu(numax=100.0)
    pgs = DevicePeriodogramBatch.from_arrays(f, power)
    with pytest.raises(ValueError, match="wider than the entire power spectrum"):
        pgs.estimate_numax(window_width=400.0)
    with pytest.raises(ValueError, match="above the highest frequency"):
        pgs.estimate_numax(numaxs=[100.0, 400.0])
    with pytest.raises(ValueError, match="below a single frequency bin"):
        pgs.estimate_numax(numaxs=[0.01, 100.0])
