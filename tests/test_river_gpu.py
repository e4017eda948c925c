"""GPU: river diagrams (cycle x phase images) against the cell-by-cell restatement of tests/river_cases.py.

Every item runs through the C ABI with host pointers (``_capi.river_batch``: ``lk_river_plan_batch`` + ``lk_river_batch``) and
through the Python API on a resident batch (``DeviceLightCurveBatch.river``: the ``_dev`` forms).  Layout, statuses, counts and
the NaN / inf pattern are exact, the median has no tolerance, mean and sigma agree within the house rule 1e-9 max(1, |ref|)
(every comparison prints its largest difference before it asserts: ``pytest -s``; DESIGN.md 4.2f records the largest measured).

``test_dyadic``: the issue that asked for this feature gives, for t = arange(64) / 8, P = 1, e = 0, bins = 8, rows 0 - 7 as
asserted below and calls row 8 empty.  By the definition it states (and by its own cadence count: 4 + 7 x 8 = 60 cadences in
rows 0 - 7 of 64) row 8 holds t = 7.5 .. 7.875: the cadence at phase -0.5 is in no column, the other three fill columns 0 - 2.
The test asserts what the definition gives for the 64 cadences, and the row that IS empty — its only cadence at phase -0.5 —
on the first 61 of them."""
import numpy as np
import pytest

import river_cases as C
from lightkurve_amd import _capi, batch as lkbatch, river as rv
from lightkurve_amd.device import DeviceLightCurveBatch
from lightkurve_amd.lightcurve import LightCurve

pytestmark = pytest.mark.gpu

METHODS = ("mean", "median", "sigma")
VIA = ("capi", "api")
_REF = {}


def ref(key, lc, **kw):
    k = (key,) + tuple(sorted(kw.items()))
    if k not in _REF:
        _REF[k] = C.reference(lc, **kw)
    return _REF[k]


def run(lcs, via, with_err=True, **kw):
    """-> (dict of to_host(), route int32[B])."""
    time, flux, err, n_off, period, epoch = C.pack(lcs, with_err)
    if via == "capi":
        out = _capi.river_batch(time, flux, n_off, period, flux_err=err, epoch_time=epoch, **kw)
        return out, out["route"]
    r = DeviceLightCurveBatch.from_arrays(time, flux, err, n_off).river(period, epoch_time=epoch, **kw)
    assert len(r) == len(lcs)
    return r.to_host(), r.routes()


def target(out, b):
    return {k: out[k][b] for k in ("river", "count", "status", "n_cycles", "n_bins")}


def check(lcs, keys, via, method, exact=False, **kw):
    out, route = run(lcs, via, method=method, **kw)
    worst = 0.0
    for b, lc in enumerate(lcs):
        kb = dict(kw, exact=exact)
        if "bins" in kb and np.ndim(kb["bins"]):
            kb["bins"] = int(kb["bins"][b])
        worst = max(worst, C.compare(target(out, b), ref(keys[b], lc, method=method, **kb), method, "%s %s" % (keys[b], via)))
    assert out["cell_off"].tolist() == np.concatenate([[0], np.cumsum([r.size for r in out["river"]])]).tolist()
    return out, route, worst


# 1 ---------------------------------------------------------------------------------------------- ragged batch
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("bin_points", [1, 4])
@pytest.mark.parametrize("method", METHODS)
def test_ragged_batch(method, bin_points, via):
    lcs = C.ragged()
    out, _, worst = check(lcs, ["ragged%d" % b for b in range(len(lcs))], via, method, bin_points=bin_points)
    assert out["status"].tolist() == [0, 1, 0, 1, 0, 0, 0, 0]
    assert out["n_cycles"][2] == 1 and out["n_cycles"][4] == 2 and out["n_cycles"][0] > 20
    print("ragged %s bin_points=%d %s: worst %.3g" % (method, bin_points, via, worst))


# 2 ---------------------------------------------------------------------------------------------- dyadic edge case
@pytest.mark.parametrize("via", VIA)
def test_dyadic(via):
    lc = C.dyadic()
    out, _, _ = check([lc], ["dyadic64"], via, "mean", bins=8, exact=True)
    river, count = out["river"][0], out["count"][0]
    assert river.shape == (9, 8)
    assert count[0].tolist() == [0, 0, 0, 1, 1, 1, 1, 0]
    assert all(count[r].tolist() == [1, 1, 1, 1, 1, 1, 1, 0] for r in range(1, 8))
    assert count[8].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]          # t = 7.5 at phase -0.5 is dropped (module docstring)
    med = np.median(lc["flux"])
    for r, j in zip(*np.nonzero(count)):
        assert river[r, j] == lc["flux"][8 * r + j - 3] / med     # exactly f / med of the single member
    assert np.isnan(river[count == 0]).all()
    assert run([lc], via)[0]["n_bins"].tolist() == [8]            # without bins: int(1 / 0.125)
    short = C.dyadic(61)                                           # row 8 holds only the cadence at phase -0.5: empty
    out, _, _ = check([short], ["dyadic61"], via, "mean", bins=8, exact=True)
    assert out["river"][0].shape == (9, 8) and not out["count"][0][8].any() and np.isnan(out["river"][0][8]).all()
    assert out["count"][0][:8].tolist() == count[:8].tolist()


# 3, 4, 6 ---------------------------------------------------------------------------------------- gap, bad values, large cells
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("method", METHODS)
def test_gap_bad_values_large_cells(method, via):
    out, _, _ = check([C.gap()], ["gap"], via, method)
    empty = np.flatnonzero(out["count"][0].sum(axis=1) == 0)
    assert empty.size >= 2 and np.isnan(out["river"][0][empty]).all()
    out, _, _ = check([C.bad_values()], ["bad"], via, method)
    if method == "sigma":
        assert np.isinf(out["river"][0]).any()                     # cells whose errors are all NaN: nansum 0, a division by zero
    out, route, _ = check([C.large_cells()], ["large"], via, method, bin_points=300)
    assert out["count"][0].max() > 64 and out["n_bins"][0] == 6
    if method == "median":
        assert route[0] & rv.ROUTE_CELL_GROUP


# 5 ---------------------------------------------------------------------------------------------- phase window, bins per target
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("method", METHODS)
def test_phase_window(method, via):
    lcs = C.window_batch()
    out, _, _ = check(lcs, ["win%d" % b for b in range(3)], via, method, minimum_phase=-0.1, maximum_phase=0.15,
                      bins=np.array([10, 37, 5]))
    assert out["n_bins"].tolist() == [10, 37, 5]
    assert np.array_equal(out["edges"][out["edge_off"][1]:out["edge_off"][2]], np.linspace(-0.1, 0.15, 38))
    check(lcs, ["win%d" % b for b in range(3)], via, method, minimum_phase=-0.1, maximum_phase=0.15, bin_points=3)
    if via == "api":
        time, flux, err, n_off, period, _ = C.pack(lcs + (C.light_curve(1, 3, 1.0),))
        r = DeviceLightCurveBatch.from_arrays(time, flux, err, n_off).river(period, minimum_phase=-0.1, maximum_phase=0.15,
                                                                            bins=[10, 37, 5, 8], method=method)
        assert np.array_equal(r.edges_of(1), np.linspace(-0.1, 0.15, 38)) and r.edges_of(3).size == 0 and r.method == method
        assert r.status.tolist() == [0, 0, 0, 1] and r.cycle_min.shape == (4,)


# 7 ---------------------------------------------------------------------------------------------- every route
@pytest.mark.parametrize("via", VIA)
def test_route_coverage(via):
    names, lcs, bins = zip(*C.route_targets())
    bins = np.array(bins)
    R = rv
    want = dict(cells_at=R.ROUTE_ROWS | R.ROUTE_VALS_LDS | R.ROUTE_CELL_THREAD,
                cells_over=R.ROUTE_COLUMNS | R.ROUTE_VALS_LDS | R.ROUTE_CELL_THREAD,
                vals_at=R.ROUTE_ROWS | R.ROUTE_VALS_LDS | R.ROUTE_CELL_GROUP,
                vals_over=R.ROUTE_ROWS | R.ROUTE_VALS_SCRATCH | R.ROUTE_CELL_GROUP,
                vals_dup=R.ROUTE_ROWS | R.ROUTE_VALS_SCRATCH | R.ROUTE_CELL_GROUP,
                cell_at=R.ROUTE_ROWS | R.ROUTE_VALS_LDS | R.ROUTE_CELL_THREAD,
                cell_over=R.ROUTE_ROWS | R.ROUTE_VALS_LDS | R.ROUTE_CELL_GROUP)
    out, route, _ = check(lcs, list(names), via, "median", bins=bins)
    got = dict(zip(names, (int(r) for r in route)))
    assert got == want
    assert np.bitwise_or.reduce(route) == 63                       # every route occurred
    sizes = dict(zip(names, (int(c.sum()) for c in out["count"])))
    assert sizes["vals_at"] == C.LDS_VALS and sizes["vals_over"] == C.LDS_VALS + 1 and sizes["vals_dup"] > C.LDS_VALS
    assert out["count"][names.index("cell_at")].max() == C.CELL_THREAD
    assert out["count"][names.index("cell_over")].max() == C.CELL_THREAD + 1
    assert out["n_bins"][:2].tolist() == [C.LDS_CELLS, C.LDS_CELLS + 1]
    for method in ("mean", "sigma"):
        _, route, _ = check(lcs, list(names), via, method, bins=bins)
        assert [int(r) for r in route] == [R.ROUTE_COLUMNS if n == "cells_over" else R.ROUTE_ROWS for n in names]


# 8 ---------------------------------------------------------------------------------------------- statuses
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("method", METHODS)
def test_statuses(method, via):
    lcs, want = zip(*C.status_batch())
    out, _, _ = check(lcs, ["status%d" % b for b in range(len(lcs))], via, method)
    assert out["status"].tolist() == list(want) and out["status"].dtype == np.int32
    for b, s in enumerate(want):
        assert (out["river"][b].size == 0) == (s != 0)
        if s == 0:                                                  # the neighbours of a bad target: as when they are alone
            alone, _ = run([lcs[b]], via, method=method)
            assert np.array_equal(alone["river"][0], out["river"][b], equal_nan=True)
            assert np.array_equal(alone["count"][0], out["count"][b])


def test_sigma_needs_errors():
    lcs = C.window_batch()
    time, flux, _, n_off, period, _ = C.pack(lcs)
    with pytest.raises(ValueError):
        _capi.river_batch(time, flux, n_off, period, method="sigma")
    with pytest.raises(ValueError):
        DeviceLightCurveBatch.from_arrays(time, flux, None, n_off).river(period, method="sigma")
    out, _ = run(lcs, "api", with_err=False, method="median", bins=12)     # a batch without flux_err serves mean and median
    for b, lc in enumerate(lcs):
        C.compare(target(out, b), ref("win%d" % b, lc, method="median", bins=12), "median", "no errors")


# 9 ---------------------------------------------------------------------------------------------- bitwise independence
@pytest.mark.parametrize("method", METHODS)
def test_bitwise_independence(method):
    T, a, b = C.ragged()[6], C.ragged()[0], C.large_cells()
    kw = dict(method=method, bin_points=2)
    alone, _ = run([T], "api", **kw)
    base = (alone["river"][0].tobytes(), alone["count"][0].tobytes())
    assert alone["river"][0].size > 500
    for lcs, at in (([T], 0), ([T, a, b], 0), ([a, T, b], 1), ([a, b, T], 2), ([a, b, T], 2)):
        for via in VIA:
            out, _ = run(lcs, via, **kw)
            assert (out["river"][at].tobytes(), out["count"][at].tobytes()) == base, (len(lcs), at, via)


# 10 --------------------------------------------------------------------------------------------- cross-check with fold
def test_row_sums_are_the_cycles_of_fold():
    lcs = [C.light_curve(1500, 31, 2.3), C.light_curve(700, 32, 0.9)]
    time, flux, err, n_off, period, _ = C.pack(lcs)
    epoch = np.array([lc["time"][0] + 0.3 for lc in lcs])
    dev = DeviceLightCurveBatch.from_arrays(time, flux, err, n_off)
    out = dev.river(period, epoch_time=epoch).to_host()
    folded = dev.fold(period, epoch_time=epoch, normalize_phase=True)
    phase, cyc = folded.to_host()["phase"], folded.cycle()
    assert np.isfinite(flux).all() and not np.any(phase == -0.5)
    for b in range(2):
        rows = np.bincount(cyc[n_off[b]:n_off[b + 1]])
        assert np.array_equal(out["count"][b].sum(axis=1), rows) and out["n_cycles"][b] == rows.size


# 11 --------------------------------------------------------------------------------------------- BLS hook, host light curves
def test_bls_hook_and_host_light_curves():
    rng = np.random.RandomState(5)
    lcs, true_p = [], (2.0, 2.3, 1.7)
    for P in true_p:
        t = 100.0 + 0.03 * np.arange(400) + 0.003 * rng.rand(400)
        f = 1.0 + 1e-4 * rng.randn(t.size)
        f[np.abs((t - 100.7 + 0.5 * P) % P - 0.5 * P) < 0.1] -= 0.01
        lcs.append(LightCurve(time=t, flux=f, flux_err=np.full(t.size, 1e-4)))
    batch = DeviceLightCurveBatch.from_lightcurves(lcs)
    res = batch.bls(np.linspace(1.6, 2.4, 81), duration=[0.2])
    pk = res.peaks()
    for method in METHODS:
        a = res.river(bins=20, method=method).to_host()
        b = batch.river(pk["period"], epoch_time=pk["transit_time"], bins=20, method=method).to_host()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["river"] + a["count"], b["river"] + b["count"]))
        assert a["status"].tolist() == [0, 0, 0] and all(r.shape[1] == 20 and r.shape[0] >= 5 for r in a["river"])
        host = lkbatch.river_batch(lcs, pk["period"], epoch_time=pk["transit_time"], bins=20, method=method)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a["river"] + a["count"], host["river"] + host["count"]))
        for i, lc in enumerate(lcs):                                # and the numpy mirror, within the house rule
            m = lc.river(pk["period"][i], epoch_time=pk["transit_time"][i], bins=20, method=method)
            assert np.array_equal(m["count"], a["count"][i])
            if method == "median":
                assert np.array_equal(m["river"], a["river"][i], equal_nan=True)
            else:
                fin = np.isfinite(m["river"])
                assert np.all(np.abs(m["river"][fin] - a["river"][i][fin]) <= 1e-9 * np.maximum(1.0, np.abs(m["river"][fin])))
