"""GPU: the under-fitting goodness metric with neighbours by index (lk_underfit_neighbors_batch*, metrics.underfit_metric_batch,
DeviceLightCurveBatch.under_fitting_metric) against the repository's own ``underfit_metric_neighbors`` per target.  Tolerance:
the house 1e-9 absolute on metric and correlations (a correct kernel is within about n 2^-53 ~ 2e-13)."""
import functools

import numpy as np
import pytest

import underfit_cases as U
from lightkurve_amd import _capi
from lightkurve_amd.correctors import metrics
from lightkurve_amd.device import DeviceLightCurveBatch

pytestmark = pytest.mark.gpu
TOL = 1e-9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def resident(y, t=None, err=None):
    """A NaN-free resident batch of the rows of y."""
    B, N = y.shape
    t = np.arange(N, dtype=np.float64) if t is None else t
    e = None if err is None else np.ascontiguousarray(err).reshape(-1)
    dev = DeviceLightCurveBatch.from_arrays(np.tile(t, B), np.ascontiguousarray(y).reshape(-1), e, np.arange(B + 1) * N)
    return dev.remove_nans()


def check(got_metric, got_corr, y, nb, cm=None, t=None):
    ref_m, ref_c = U.mirror(y, nb, cm, t)
    nb = np.asarray(nb).reshape(len(y), -1)
    err_m = np.max(np.abs(got_metric - ref_m)) if len(ref_m) else 0.0
    pad = nb < 0
    assert got_corr.shape == nb.shape and np.array_equal(np.isnan(got_corr), pad)
    err_c = np.max(np.abs(got_corr[~pad] - ref_c[~pad])) if (~pad).any() else 0.0
    print("max |metric - mirror| %.3e   max |corr - mirror| %.3e" % (err_m, err_c))
    assert err_m < TOL and err_c < TOL
    return ref_m


@functools.lru_cache(maxsize=None)
def reference_run(cfg):
    """One run of the host-pointer entry point per configuration, shared by the tests that compare against it."""
    f = U.field(*cfg)
    r = _capi.underfit_neighbors_batch(f["y"], f["neighbors"], cadence_mask=f["cm"])
    r["metric"].setflags(write=False)
    r["correlations"].setflags(write=False)
    return r


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("cfg", U.CONFIGS)
def test_parity_with_the_mirror_through_the_three_front_ends(cfg):
    f = U.field(*cfg)
    y, nb, cm, t = f["y"], f["neighbors"], f["cm"], f["t"]
    r = reference_run(cfg)
    ref_m = check(r["metric"], r["correlations"], y, nb, cm, t)
    assert np.median(ref_m) < 0.6 and np.median(r["metric"]) < 0.6          # raw flux: strongly under-fitted
    m2, c2 = metrics.underfit_metric_batch(y, nb, cadence_mask=cm, return_correlations=True)
    m3, c3 = resident(y, t).under_fitting_metric(nb, cadence_mask=cm, return_correlations=True)
    assert same_bits(m2, r["metric"]) and same_bits(c2, r["correlations"])
    assert same_bits(m3, r["metric"]) and same_bits(c3, r["correlations"])
    assert same_bits(metrics.underfit_metric_batch(y, nb, cadence_mask=cm), r["metric"])
    assert same_bits(resident(y, t).under_fitting_metric(nb, cadence_mask=cm), r["metric"])


# ------------------------------------------------------------------------------------------------ 2. row tails, alignment
@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 127, 128, 129, 255, 257, 2049])
def test_row_tails_without_a_mask(N):
    """B = 5 and no mask: rows of odd N start off 16-byte alignment in the flux, and every N ends a 128-element step elsewhere."""
    f = U.field(30 + N, 5, N, 4)
    r = _capi.underfit_neighbors_batch(f["y"], f["neighbors"])
    check(r["metric"], r["correlations"], f["y"], f["neighbors"])
    m, c = resident(f["y"]).under_fitting_metric(f["neighbors"], return_correlations=True)
    assert same_bits(m, r["metric"]) and same_bits(c, r["correlations"])


@pytest.mark.parametrize("drop", [[0, 5, 64, 128], [1, 77, 256]])
def test_even_and_odd_kept_counts_under_a_mask(drop):
    """N = 257 less four cadences = 253 (odd: the median is one element), less three = 254 (even: the mean of two)."""
    f = U.field(77, 5, 257, 4)
    cm = np.ones(257, dtype=bool)
    cm[drop] = False
    assert cm.sum() % 2 == len(drop) % 2 ^ 1
    r = _capi.underfit_neighbors_batch(f["y"], f["neighbors"], cadence_mask=cm)
    check(r["metric"], r["correlations"], f["y"], f["neighbors"], cm)
    m, c = resident(f["y"]).under_fitting_metric(f["neighbors"], cadence_mask=cm, return_correlations=True)
    assert same_bits(m, r["metric"]) and same_bits(c, r["correlations"])


# ------------------------------------------------------------------------------------------------ 3. neighbour lists
def test_padding_single_neighbour_and_no_neighbours():
    f = U.field(*U.CONFIGS[3])
    y, cm = f["y"], f["cm"]
    nb = f["neighbors"].copy()
    nb[0, 1:] = -1           # one neighbour
    nb[1, :] = -1            # none: metric exactly 1, correlations NaN
    nb[2, ::2] = -1          # padding in between
    nb[3, :3] = -1           # padding in front
    r = _capi.underfit_neighbors_batch(y, nb, cadence_mask=cm)
    check(r["metric"], r["correlations"], y, nb, cm)
    assert r["metric"][1] == 1.0 and np.all(np.isnan(r["correlations"][1]))
    # M = 0
    none = np.zeros((len(y), 0), dtype=np.int32)
    r0 = _capi.underfit_neighbors_batch(y, none, cadence_mask=cm)
    assert r0["correlations"].shape == (len(y), 0) and np.all(r0["metric"] == 1.0)
    m0, c0 = resident(y).under_fitting_metric(none, cadence_mask=cm, return_correlations=True)
    assert c0.shape == (len(y), 0) and np.all(m0 == 1.0)
    # M = 1
    r1 = _capi.underfit_neighbors_batch(y, f["neighbors"][:, :1], cadence_mask=cm)
    check(r1["metric"], r1["correlations"], y, f["neighbors"][:, :1], cm)


def test_more_neighbours_than_one_trip_of_the_wavefronts():
    """M = 70 on B = 80: three trips of 32 list positions, the last one partly filled."""
    cfg = U.CONFIGS[2]
    assert cfg[1] == 80 and cfg[3] == 70
    f = U.field(*cfg)
    r = reference_run(cfg)
    check(r["metric"], r["correlations"], f["y"], f["neighbors"], f["cm"], f["t"])
    nb = f["neighbors"][:, :33]       # one position into the second trip
    r2 = _capi.underfit_neighbors_batch(f["y"], nb, cadence_mask=f["cm"])
    check(r2["metric"], r2["correlations"], f["y"], nb, f["cm"], f["t"])
    assert same_bits(r2["correlations"], r["correlations"][:, :33])


def test_duplicated_neighbour_equals_the_mirror_with_the_column_repeated():
    f = U.field(*U.CONFIGS[1])
    nb = f["neighbors"].copy()
    nb[:, 2] = nb[:, 0]
    r = _capi.underfit_neighbors_batch(f["y"], nb, cadence_mask=f["cm"])
    check(r["metric"], r["correlations"], f["y"], nb, f["cm"], f["t"])      # (the mirror gets the column twice)
    assert same_bits(r["correlations"][:, 2], r["correlations"][:, 0])


def test_constant_flux_target_and_constant_flux_neighbour():
    f = U.field(*U.CONFIGS[3])
    y = f["y"].copy()
    y[4, :] = 1234.5                   # z == 0 exactly: rms 0 -> the mirror's rms = inf rule
    nb = f["neighbors"]                # every other target is a neighbour, so 4 is a neighbour of all the rest
    r = _capi.underfit_neighbors_batch(y, nb, cadence_mask=f["cm"])
    check(r["metric"], r["correlations"], y, nb, f["cm"], f["t"])
    assert np.all(bits(r["correlations"][4]) == 0) and r["metric"][4] == 1.0
    assert np.all(bits(r["correlations"][nb == 4]) == 0)


# ------------------------------------------------------------------------------------------------ 4. order independence
def test_mutual_neighbours_see_the_same_bits():
    for cfg in (U.CONFIGS[3], U.CONFIGS[2]):
        f = U.field(*cfg)
        nb, c = f["neighbors"], reference_run(cfg)["correlations"]
        pairs = 0
        for t in range(len(nb)):
            for p, j in enumerate(nb[t]):
                back = np.nonzero(nb[j] == t)[0]
                if len(back):
                    pairs += 1
                    assert bits(c[t, p]) == bits(c[j, back[0]]), (t, j)
        assert pairs > 50


def test_permuting_a_row_permutes_the_correlations_bit_for_bit():
    cfg = U.CONFIGS[2]
    f = U.field(*cfg)
    base = reference_run(cfg)["correlations"]
    nb = f["neighbors"].copy()
    perm = np.random.default_rng(1).permutation(nb.shape[1])
    nb[3] = nb[3][perm]
    nb[7] = nb[7][::-1]
    r = _capi.underfit_neighbors_batch(f["y"], nb, cadence_mask=f["cm"])
    assert same_bits(r["correlations"][3], base[3][perm]) and same_bits(r["correlations"][7], base[7][::-1])
    untouched = np.delete(np.arange(len(nb)), [3, 7])
    assert same_bits(r["correlations"][untouched], base[untouched])


def test_a_sub_batch_gives_the_same_bits():
    cfg = U.CONFIGS[0]
    f = U.field(*cfg)
    full = reference_run(cfg)
    for t in (0, 17, 36):
        idx = np.concatenate([[t], f["neighbors"][t]])
        sub_nb = np.full((len(idx), len(idx) - 1), -1, dtype=np.int32)
        sub_nb[0] = np.arange(1, len(idx))
        r = _capi.underfit_neighbors_batch(f["y"][idx], sub_nb, cadence_mask=f["cm"])
        assert same_bits(r["correlations"][0], full["correlations"][t]) and bits(r["metric"][0]) == bits(full["metric"][t])


def test_two_runs_are_equal():
    cfg = U.CONFIGS[2]
    f = U.field(*cfg)
    a = reference_run(cfg)
    b = _capi.underfit_neighbors_batch(f["y"], f["neighbors"], cadence_mask=f["cm"])
    assert same_bits(a["metric"], b["metric"]) and same_bits(a["correlations"], b["correlations"])


# ------------------------------------------------------------------------------------------------ 5. chain
def test_cbv_correct_then_under_fitting_metric_stays_resident():
    cfg = U.CONFIGS[0]
    f = U.field(*cfg)
    y, nb, cm, t, S = f["y"], f["neighbors"], f["cm"], f["t"], f["S"]
    B, N = y.shape
    dev = resident(y, t, err=1e-3 * y)
    corrected, _d_outl, _d_w = dev.cbv_correct(S, cbv_indices=[1, 2], cadence_mask=np.broadcast_to(cm, (B, N)), to_host=False)
    d_metric, d_corr = corrected.under_fitting_metric(nb, cadence_mask=cm, return_correlations=True, to_host=False)
    # one download at the end
    metric = d_metric.download(np.float64, B, stream=corrected.stream)
    corr = d_corr.download(np.float64, nb.size, stream=corrected.stream).reshape(nb.shape)
    flux = corrected.flux_host().reshape(B, N)
    check(metric, corr, flux, nb, cm, t)
    print("min metric after cbv_correct %.4f, median before %.4f" % (metric.min(), np.median(reference_run(cfg)["metric"])))
    assert metric.min() > 0.99 and np.median(reference_run(cfg)["metric"]) < 0.6


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_are_raised_before_any_launch():
    f = U.field(*U.CONFIGS[3])
    y, nb, t = f["y"], f["neighbors"], f["t"]
    B, N = y.shape
    ragged = DeviceLightCurveBatch.from_arrays(np.arange(2 * N - 5, dtype=np.float64), np.ones(2 * N - 5), None, [0, N, 2 * N - 5])
    with pytest.raises(ValueError, match="one cadence count"):
        ragged.remove_nans().under_fitting_metric([[1], [0]])
    unmarked = DeviceLightCurveBatch.from_arrays(np.tile(t, B), y.reshape(-1), None, np.arange(B + 1) * N)
    with pytest.raises(ValueError, match=r"remove_nans\(\)"):
        unmarked.under_fitting_metric(nb)
    dev = resident(y, t)
    bad = nb.copy()
    bad[2, 1] = B
    with pytest.raises(ValueError, match=r"index in \[0, %d\)" % B):
        dev.under_fitting_metric(bad)
    bad = nb.copy()
    bad[2, 1] = 2
    with pytest.raises(ValueError, match="its own neighbour"):
        dev.under_fitting_metric(bad)
    with pytest.raises(ValueError, match=r"shape \(%d,\)" % N):
        dev.under_fitting_metric(nb, cadence_mask=np.ones(N + 1, dtype=bool))
    one = np.zeros(N, dtype=bool)
    one[5] = True
    with pytest.raises(ValueError, match="at least two kept cadences"):
        dev.under_fitting_metric(nb, cadence_mask=one)
    # the C ABI's own checks (status 1 -> ValueError) behind the Python ones
    h = _capi.Handle.get(0)
    z = np.zeros(4)
    ip = _capi._c_i32p
    self_nb = np.array([[0], [0]], dtype=np.int32)
    for args in ((0, 2, 2, None, 0, None), (2, 2, 1, None, 0, None), (2, 2, 3, None, 0, None), (2, 2, 2, None, -1, None),
                 (2, 2, 2, None, 1, self_nb)):
        Bc, Nc, nc, keep, Mc, nbc = args
        rc = _capi._lib.lk_underfit_neighbors_batch(h._h, Bc, Nc, _capi._ptr(z), nc, keep, Mc, _capi._ptr(nbc, ip), None, _capi._ptr(z))
        assert rc == _capi.LK_EINVAL, args
