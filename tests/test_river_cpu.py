"""CPU: the host side of the river diagrams — ``LightCurve.river`` (the numpy mirror) and ``river.py``'s statuses and layout
against the cell-by-cell restatement of tests/river_cases.py, the n_bins expression, every ``ValueError``, every status and
``max_output_mb``.  No GPU."""
import os
import re

import numpy as np
import pytest

import river_cases as C
from lightkurve_amd import river as rv
from lightkurve_amd.lightcurve import LightCurve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("mean", "median", "sigma")


def mirror(lc, **kw):
    return LightCurve(time=lc["time"], flux=lc["flux"], flux_err=lc["flux_err"]).river(lc["period"], epoch_time=lc["epoch"], **kw)


def test_constants_mirror_the_header():
    src = open(os.path.join(ROOT, "include", "lkhip.h")).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))
    assert (rv.NPLAN, rv.LDS_CELLS, rv.LDS_VALS, rv.CELL_THREAD) == tuple(
        val("LK_RIVER_" + k) for k in ("NPLAN", "LDS_CELLS", "LDS_VALS", "CELL_THREAD"))
    assert (C.LDS_CELLS, C.LDS_VALS, C.CELL_THREAD) == (rv.LDS_CELLS, rv.LDS_VALS, rv.CELL_THREAD)
    for k in ("ROWS", "COLUMNS", "VALS_LDS", "VALS_SCRATCH", "CELL_THREAD", "CELL_GROUP"):
        assert getattr(rv, "ROUTE_" + k) == val("LK_RIVER_ROUTE_" + k)
    assert rv.METHODS == {"mean": 0, "median": 1, "sigma": 2}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("bin_points", [1, 4])
def test_mirror_ragged(method, bin_points):
    for b, lc in enumerate(C.ragged()):
        C.compare(mirror(lc, bin_points=bin_points, method=method), C.reference(lc, bin_points=bin_points, method=method), method,
                  "ragged[%d] bin_points=%d" % (b, bin_points))
    got = [mirror(lc)["n_cycles"] for lc in C.ragged()]
    assert got[2] == 1 and got[4] == 2 and got[0] > 20 and got[1] == got[3] == 0


def test_mirror_dyadic_edges():
    lc = C.dyadic()
    got = mirror(lc, bins=8)
    C.compare(got, C.reference(lc, bins=8, exact=True), "mean", "dyadic")
    assert got["river"].shape == (9, 8)
    assert got["count"][0].tolist() == [0, 0, 0, 1, 1, 1, 1, 0]
    assert all(got["count"][r].tolist() == [1, 1, 1, 1, 1, 1, 1, 0] for r in range(1, 8))
    # the last row of 64 cadences holds t = 7.5 (phase -0.5: in no column) .. 7.875 — see test_river_gpu.test_dyadic
    assert got["count"][8].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    med = np.median(lc["flux"])
    for r, j in zip(*np.nonzero(got["count"])):
        k = int(round((r + (j - 3) / 8.0) * 8))                  # the one member: t = r + edges[j + 1]
        assert got["river"][r, j] == lc["flux"][k] / med
    assert mirror(lc)["n_bins"] == 8                             # int(1 / 0.125 * 1 / 1)
    short = mirror(C.dyadic(61), bins=8)                         # the last row holds only the cadence at phase -0.5: empty
    assert short["river"].shape == (9, 8) and not short["count"][8].any() and np.isnan(short["river"][8]).all()


@pytest.mark.parametrize("method", METHODS)
def test_mirror_gap_bad_values_large_cells(method):
    lc = C.gap()
    got = mirror(lc, method=method)
    C.compare(got, C.reference(lc, method=method), method, "gap")
    empty = np.flatnonzero(got["count"].sum(axis=1) == 0)
    assert empty.size >= 2 and np.isnan(got["river"][empty]).all()
    C.compare(mirror(C.bad_values(), method=method), C.reference(C.bad_values(), method=method), method, "bad values")
    C.compare(mirror(C.large_cells(), bin_points=300, method=method), C.reference(C.large_cells(), bin_points=300, method=method),
              method, "large cells")
    assert C.reference(C.large_cells(), bin_points=300)["count"].max() > 64


def test_mirror_window_and_bins():
    for lc, bins in zip(C.window_batch(), (10, 37, 5)):
        kw = dict(minimum_phase=-0.1, maximum_phase=0.15, bins=bins)
        got = mirror(lc, **kw)
        C.compare(got, C.reference(lc, **kw), "mean", "window")
        assert np.array_equal(got["edges"], np.linspace(-0.1, 0.15, bins + 1))
    lc = C.window_batch()[0]
    kw = dict(minimum_phase=-0.1, maximum_phase=0.15, bin_points=3)
    C.compare(mirror(lc, **kw), C.reference(lc, **kw), "mean", "window without bins")


def test_n_bins_expression():
    assert rv.n_bins_of(1.0, 0.125) == 8
    for P, dt, bp, lo, hi in ((3.7, 0.0204, 1, -0.5, 0.5), (3.7, 0.0204, 4, -0.5, 0.5), (2.3, 0.0207, 3, -0.1, 0.15), (0.01, 0.02, 1, -0.5, 0.5)):
        assert rv.n_bins_of(P, dt, bp, lo, hi) == int(P / dt * (hi - lo) / bp)
    assert rv.n_bins_of(0.3, 0.1) == int(0.3 / 0.1 * 1.0 / 1)    # 2, not 3: the order of the operations is the contract


def test_value_errors():
    lc = C.ragged()[6]
    for kw in (dict(bin_points=0), dict(bin_points=1.5), dict(minimum_phase=-0.6), dict(maximum_phase=0.51),
               dict(minimum_phase=0.2, maximum_phase=0.2), dict(minimum_phase=0.3, maximum_phase=0.1), dict(bins=0), dict(bins=-3),
               dict(bins=2.5), dict(method="max")):
        with pytest.raises(ValueError):
            mirror(lc, **kw)
    for P in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            LightCurve(time=lc["time"], flux=lc["flux"]).river(P)
    with pytest.raises(ValueError):
        rv.check_arguments(3, 1.0, method="sigma", has_err=False)
    with pytest.raises(ValueError):
        rv.river_numpy(lc["time"], lc["flux"], None, lc["period"], method="sigma")
    with pytest.raises(ValueError):
        rv.check_arguments(3, [1.0, 2.0, -1.0])
    with pytest.raises(ValueError):
        rv.check_arguments(3, 1.0, bins=[4, 0, 4])


def test_statuses():
    for lc, want in C.status_batch():
        got = mirror(lc)
        assert got["status"] == want == C.expected_status(lc)
        if want:
            assert got["river"].shape == (0, 0) and got["count"].shape == (0, 0) and got["n_bins"] == got["n_cycles"] == 0
    lc = C.light_curve(100, 5, 1.0)
    lc["flux"][:] = np.nan
    assert mirror(lc)["status"] == 1
    lc = C.light_curve(100, 5, 1.0)
    lc["time"][40] = np.inf
    assert mirror(lc)["status"] == 2
    lc = C.light_curve(100, 5, 1.0)
    lc["time"][:] = lc["time"][0]
    assert mirror(lc)["status"] == 3                              # median step 0


def test_layout_of_a_batch():
    lcs = [lc for lc, _ in C.status_batch()]
    B = len(lcs)
    period = np.array([lc["period"] for lc in lcs])
    plan = np.stack([rv.plan_numpy(lc["time"], lc["flux"], lc["flux_err"], lc["period"]) for lc in lcs])
    lay = rv.layout([lc["time"].size for lc in lcs], plan, period)
    refs = [C.reference(lc) for lc in lcs]
    assert lay["status"].tolist() == [s for _, s in C.status_batch()] and lay["status"].dtype == np.int32
    assert lay["n_bins"].tolist() == [r["n_bins"] for r in refs] and lay["n_cycles"].tolist() == [r["n_cycles"] for r in refs]
    assert lay["cell_off"].tolist() == np.concatenate([[0], np.cumsum([r["river"].size for r in refs])]).tolist()
    assert lay["edge_off"].tolist() == np.concatenate([[0], np.cumsum([r["n_bins"] + 1 for r in refs])]).tolist()
    for b in range(B):
        if refs[b]["status"] == 0:
            assert np.array_equal(lay["edges"][lay["edge_off"][b]:lay["edge_off"][b + 1]], refs[b]["edges"])
    flat = np.arange(lay["cell_off"][-1], dtype=np.float64)
    parts = rv.split(flat, lay)
    assert [p.shape for p in parts] == [r["river"].shape for r in refs] and parts[2][1, 0] == lay["cell_off"][2] + lay["n_bins"][2]


def test_max_output_mb():
    lc = C.ragged()[0]
    cells = C.reference(lc)["river"].size
    need = cells * 12 / 2.0 ** 20
    assert mirror(lc, max_output_mb=need * 1.01)["status"] == 0
    with pytest.raises(ValueError, match="max_output_mb"):
        mirror(lc, max_output_mb=need * 0.99)
    long = dict(C.light_curve(3000, 3, 0.05, cadence=2.0))       # 16 years at a period of 0.05 d with 10^6 bins: 10^11 cells
    with pytest.raises(ValueError, match="max_output_mb"):
        mirror(long, bins=10 ** 6)


def test_public_interface_exists():
    from lightkurve_amd import _capi, batch
    from lightkurve_amd.device import DeviceBLSResult, DeviceLightCurveBatch, DeviceRiverBatch
    assert callable(DeviceLightCurveBatch.river) and callable(DeviceBLSResult.river) and callable(batch.river_batch)
    assert callable(_capi.river_batch) and callable(DeviceRiverBatch.to_host)
    names = [s[0] for s in _capi.SIGNATURES]
    assert all(n in names for n in ("lk_river_plan_batch", "lk_river_plan_batch_dev", "lk_river_batch", "lk_river_batch_dev"))
