"""correctors.cbvcorrector.interpolate_cbvs (the numpy mirror of CotrendingBasisVectors.interpolate and of
lk_pchip_interp_batch) against scipy.interpolate.PchipInterpolator, and the C ABI's new symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

import scipy.interpolate as scipy_interpolate

from lightkurve_amd.correctors.cbvcorrector import interpolate_cbvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9      # of the column's largest |value| (the house rule; about 5e-16 is what the restatement gives)


def knots(Nx, K, seed):
    """Uneven strictly increasing knot times and K columns with flat runs (zero secants), sign changes of the secant and
    one steep step (so the end conditions and the harmonic mean see every branch)."""
    rng = np.random.default_rng(seed)
    x = 1000.0 + np.cumsum(rng.uniform(0.5, 1.5, Nx)) / 720.0
    y = np.cumsum(rng.normal(0, 1, (Nx, K)), axis=0) + 3.0 * np.sin(np.arange(Nx)[:, None] / 3.0 + np.arange(K))
    if Nx >= 4:
        y[Nx // 3:Nx // 3 + max(2, Nx // 10), 0] = y[Nx // 3, 0]        # a flat run
        y[-2:, K - 1] = y[-3, K - 1]                                     # flat at the end
    if Nx >= 50:
        y[Nx // 2:, K // 2] += 40.0                                      # a step
    return x, y


def queries(x, seed):
    """Between the knots, on the first / an interior / the last knot (bit-equal), outside both ends, NaN."""
    rng = np.random.default_rng(seed + 100)
    span = x[-1] - x[0]
    t = np.sort(rng.uniform(x[0] - 0.05 * span, x[-1] + 0.05 * span, 4 * x.size + 7))
    extra = np.array([x[0], x[x.size // 2], x[-1], x[0] - 0.3 * span, x[-1] + 0.3 * span, np.nextafter(x[0], -np.inf),
                      np.nextafter(x[-1], np.inf), np.nan])
    return np.concatenate([t, extra])


def scipy_ref(x, y, t, extrapolate):
    return scipy_interpolate.PchipInterpolator(x, y, axis=0, extrapolate=extrapolate)(t)


@pytest.mark.parametrize("extrapolate", [False, True])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("Nx", [2, 3, 4, 50, 1200])
def test_interpolate_cbvs_matches_scipy(Nx, K, extrapolate):
    x, y = knots(Nx, K, Nx + K)
    t = queries(x, Nx)
    got = interpolate_cbvs(x, y, t, extrapolate=extrapolate)
    ref = scipy_ref(x, y, t, extrapolate)
    assert got.shape == ref.shape == (t.size, K)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    if not extrapolate:
        assert np.array_equal(np.isnan(got[:, 0]), ~((t >= x[0]) & (t <= x[-1])))
    ok = ~np.isnan(ref)
    scale = np.abs(np.where(ok, ref, 0.0)).max(axis=0)
    err = np.abs(np.where(ok, got - ref, 0.0)).max(axis=0) / scale
    print("Nx=%d K=%d extrapolate=%s: max error / column scale %.2e" % (Nx, K, extrapolate, err.max()))
    assert err.max() < TOL


@pytest.mark.parametrize("Nx", [2, 3, 4, 50, 1200])
def test_query_on_a_knot_returns_the_knot_bit_for_bit(Nx):
    x, y = knots(Nx, 5, Nx)
    for extrapolate in (False, True):
        got = interpolate_cbvs(x, y, x.copy(), extrapolate=extrapolate)
        assert np.array_equal(got, y)


@pytest.mark.parametrize("extrapolate", [False, True])
def test_gap_indicators_remove_knots(extrapolate):
    x, y = knots(60, 3, 7)
    gap = np.zeros(60, dtype=bool)
    gap[[0, 59]] = True
    gap[20:31] = True
    y[gap] = np.nan                # what a gap-flagged CBV cadence may hold: never looked at
    t = queries(x, 3)
    got = interpolate_cbvs(x, y, t, gap_indicators=gap, extrapolate=extrapolate)
    ref = scipy_ref(x[~gap], y[~gap], t, extrapolate)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert (np.abs(np.where(ok, got - ref, 0.0)).max(axis=0) / np.abs(np.where(ok, ref, 0.0)).max(axis=0)).max() < TOL
    kept = interpolate_cbvs(x, y, x[~gap], gap_indicators=gap)
    assert np.array_equal(kept, y[~gap])
    if not extrapolate:             # the span is the kept knots' span: the removed first and last knots are outside
        assert np.all(np.isnan(interpolate_cbvs(x, y, x[[0, 59]], gap_indicators=gap)))


def test_argument_errors():
    x, y = knots(10, 2, 1)
    t = x[:3]
    with pytest.raises(ValueError, match="strictly increasing"):
        interpolate_cbvs(x[::-1], y, t)
    xr = x.copy()
    xr[4] = xr[3]
    with pytest.raises(ValueError, match="strictly increasing"):
        interpolate_cbvs(xr, y, t)
    xn = x.copy()
    xn[5] = np.nan
    with pytest.raises(ValueError, match="finite"):
        interpolate_cbvs(xn, y, t)
    gap = np.ones(10, dtype=bool)
    gap[3] = False
    with pytest.raises(ValueError, match="at least 2"):
        interpolate_cbvs(x, y, t, gap_indicators=gap)
    yn = y.copy()
    yn[2, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        interpolate_cbvs(x, yn, t)
    with pytest.raises(ValueError, match="at least one column"):
        interpolate_cbvs(x, y[:, :0], t)
    with pytest.raises(ValueError, match="one row per CBV cadence"):
        interpolate_cbvs(x, y[:-1], t)
    with pytest.raises(ValueError, match="gap_indicators"):
        interpolate_cbvs(x, y, t, gap_indicators=np.zeros(9, dtype=bool))
    with pytest.raises(ValueError, match="1-D"):
        interpolate_cbvs(x, y, t[:, None])


def test_the_interpolated_route_excludes_the_aligned_ones_before_any_device_call():
    from lightkurve_amd import device as D
    b = object.__new__(D.DeviceLightCurveBatch)
    b.n_off = np.asarray([0, 100, 190], dtype=np.int64)
    b.d_cadenceno = object()
    X, x, grid = np.ones((50, 3)), np.arange(50.0), np.arange(50)
    with pytest.raises(ValueError, match="cannot be combined"):
        b.regression_correct(X, knot_time=x, cadenceno=grid)
    with pytest.raises(ValueError, match="cannot be combined"):
        b.regression_correct(X, knot_time=x, rows=np.zeros(190, dtype=np.int64))
    with pytest.raises(ValueError, match="cannot be combined"):
        b.cbv_correct(np.ones((50, 16)), cbv_time=x, cadenceno=grid)
    with pytest.raises(ValueError, match="pass `knot_time`"):
        b.regression_correct(X, cadenceno=grid, extrapolate=True)
    with pytest.raises(ValueError, match="pass `cbv_time`"):
        b.cbv_correct(np.ones((50, 16)), cadenceno=grid, gap_indicators=np.zeros(50, dtype=bool))
    with pytest.raises(ValueError, match=r"knot times must be a real array of shape \(50,\)"):
        b.regression_correct(X, knot_time=x[:-1])
    with pytest.raises(ValueError, match=r"knot mask must be a bool array of shape \(50,\)"):
        b.regression_correct(X, knot_time=x, knot_keep=np.ones(49, dtype=bool))
    with pytest.raises(ValueError, match="at least 2 knots"):
        b.cbv_correct(np.ones((50, 16)), cbv_time=x, gap_indicators=np.arange(50) > 0)
    from lightkurve_amd.correctors.designmatrix import DesignMatrix
    with pytest.raises(ValueError, match="`ext_dm` is not interpolated"):
        b.cbv_correct(np.ones((50, 16)), cbv_time=x, ext_dm=DesignMatrix(np.ones((50, 1))))
    b.n_off = np.asarray([0, 100, 190], dtype=np.int64)
    with pytest.raises(ValueError, match=r"cadence_mask is ragged.*shape \(190,\)"):
        b.cbv_correct(np.ones((50, 16)), cbv_time=x, cadence_mask=np.ones((2, 95), dtype=bool))


def test_capi_declares_the_interpolation():
    """Header and ctypes table agree on the two entry points and their argument counts."""
    from lightkurve_amd import _capi
    text = open(os.path.join(ROOT, "include", "lkhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    table = {s[0]: s for s in _capi.SIGNATURES}
    for name, nargs in (("lk_pchip_interp_batch", 13), ("lk_pchip_interp_batch_dev", 14)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m is not None and name in table, name
        assert len(m.group(1).split(",")) == nargs == len(table[name][2]), name
