"""CPU: the under-fitting metric of ragged batches on a cadence grid — the numpy closed form of the grid kernels against the
repository's ``underfit_metric_neighbors`` fed as the reference would feed it, the C ABI's declarations, and the Python checks that
must raise before any device call (none of these needs a GPU)."""
import os
import re

import numpy as np
import pytest

import ragged_goodness_cases as R
from lightkurve_amd import _capi
from lightkurve_amd.correctors import metrics
from lightkurve_amd.device import DeviceLightCurveBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
NEW = ["lk_underfit_grid_neighbors_batch", "lk_underfit_grid_neighbors_batch_dev", "lk_underfit_grid_rows_bytes",
       "lk_underfit_grid_rows_prepare_dev", "lk_underfit_grid_against_rows_batch_dev", "lk_overfit_scratch_rows_bytes",
       "lk_overfit_metric_rows_batch", "lk_overfit_metric_rows_batch_dev", "lk_overfit_session_rows_bytes",
       "lk_overfit_session_begin_rows_dev", "lk_overfit_session_eval_rows_dev"]


@pytest.mark.parametrize("cfg", R.CONFIGS)
def test_closed_form_equals_the_mirror(cfg):
    f = R.ragged_field(*cfg)
    present = f["has"] & f["cm"][None, :]
    ref_m, ref_c, ref_n = R.reference(cfg)
    m, c, n = R.closed_form(f["y"], present, f["neighbors"])
    Nx = cfg[2]
    print("n_common min %d of %d, median raw metric %.3f" % (ref_n.min(), Nx, np.median(ref_m)))
    assert np.array_equal(n, ref_n) and ref_n.min() >= 0.6 * Nx and ref_n.max() < present.sum(axis=1).max() + 1
    assert (ref_n < present.sum(axis=1)).any()                  # the intersection really is smaller than a target's own set
    assert np.max(np.abs(m - ref_m)) < TOL and np.max(np.abs(c - ref_c)) < TOL
    if cfg[0] in (21, 22, 23):
        assert np.median(ref_m) < 0.5
    det_m, det_c, det_n = R.reference(cfg, True)
    assert det_m.min() > 0.99 and np.array_equal(det_n, ref_n)
    from underfit_cases import detrended
    m2, c2, _ = R.closed_form(detrended(f["y"], f["S"], f["cm"]), present, f["neighbors"])
    assert np.max(np.abs(m2 - det_m)) < TOL and np.max(np.abs(c2 - det_c)) < TOL


def test_closed_form_edge_rules():
    y = 1000.0 + np.arange(24, dtype=np.float64).reshape(3, 8) ** 2
    has = np.ones((3, 8), dtype=bool)
    has[0, 4:] = False
    has[1, :4] = False                                           # 0 and 1 are disjoint
    nb = np.array([[1, -1], [-1, -1], [0, 1]], dtype=np.int32)
    m, c, n = R.closed_form(y, has, nb)
    assert n.tolist() == [0, 4, 0] and np.isnan(m[0]) and m[1] == 1.0 and np.isnan(m[2]) and np.all(np.isnan(c))


def test_new_symbols_are_declared_with_matching_arguments():
    """Every new entry point: declared in include/lkhip.h, listed in _capi.SIGNATURES with as many arguments, and the ctypes kinds
    (pointer / int / int64) agree with the C declaration."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lkhip.h")).read(), flags=re.S)
    table = {s[0]: s for s in _capi.SIGNATURES}
    import ctypes
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, "%s is not declared in lkhip.h" % name
        assert name in table, "%s is not in _capi.SIGNATURES" % name
        cargs = [a.strip() for a in m.group(1).split(",")]
        pyargs = table[name][2]
        assert len(cargs) == len(pyargs), (name, len(cargs), len(pyargs))
        for ca, pa in zip(cargs, pyargs):
            if "*" in ca:
                assert pa is ctypes.c_void_p or hasattr(pa, "_type_") and not isinstance(pa._type_, str), (name, ca, pa)
            elif ca.startswith("int64_t"):
                assert pa is ctypes.c_int64, (name, ca, pa)
            elif ca.startswith("uint64_t"):
                assert pa is ctypes.c_uint64, (name, ca, pa)
            elif ca.startswith("double"):
                assert pa is ctypes.c_double, (name, ca, pa)
            else:
                assert ca.startswith("int ") and pa is ctypes.c_int, (name, ca, pa)
    for f in ("underfit_metric_ragged_batch", "overfit_metric_ragged_batch"):
        assert hasattr(metrics, f) and f in metrics.__all__


def test_kept_cadences_of_a_ragged_mask():
    n_off = np.array([0, 5, 9, 12])
    cm = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1], dtype=bool)
    keep_idx, k_off, grid = _capi.overfit_rows_arguments(n_off, 1, cm, [0.5, 1.0, 1.5])
    assert keep_idx.dtype == np.int32 and keep_idx.tolist() == [0, 2, 3, 0, 1, 2, 0, 1, 2] and k_off.tolist() == [0, 3, 6, 9]
    assert grid[2] == 3
    keep_idx, k_off, grid = _capi.overfit_rows_arguments(n_off, 1, None, None)
    assert keep_idx is None and k_off.tolist() == n_off.tolist() and grid is None
    cm[9] = False
    with pytest.raises(ValueError, match="target 2: .*at least three kept cadences \\(got 2\\)"):
        _capi.overfit_rows_arguments(n_off, 1, cm, None)
    with pytest.raises(ValueError, match="target 1: .*at least three"):
        _capi.overfit_rows_arguments([0, 5, 7, 12], 1, None, None)


class _NoDevice(object):
    """Stands where the C library would: any call through it is a device call that came too early."""

    def __getattr__(self, name):
        raise AssertionError("device call %s before the argument checks were done" % name)


def _host_batch(n_off, cadenceno=True, nan_free=True):
    """A DeviceLightCurveBatch object that owns no device memory: enough for the checks that run before any device call."""
    n_off = np.asarray(n_off, dtype=np.int64)
    b = DeviceLightCurveBatch.__new__(DeviceLightCurveBatch)
    b.n_off, b.nan_free, b.is_sorted, b.stream, b.meta, b._keep = n_off, nan_free, True, 0, [dict() for _ in n_off[1:]], []
    b.d_time = b.d_flux = b.d_flux_err = object()
    b.d_cadenceno = object() if cadenceno else None
    b.handle = _NoDevice()
    return b


def test_python_checks_raise_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_capi, "_lib", _NoDevice())
    grid = np.arange(100, 140, dtype=np.int32)
    nb = np.array([[1], [0]], dtype=np.int32)
    ragged = _host_batch([0, 30, 55])
    assert ragged.n_cadences == 55 and len(ragged) == 2
    with pytest.raises(ValueError, match="carries cadence numbers"):
        _host_batch([0, 30, 55], cadenceno=False).under_fitting_metric(nb, cadenceno=grid)
    with pytest.raises(ValueError, match="strictly increasing"):
        ragged.under_fitting_metric(nb, cadenceno=grid[::-1].copy())
    with pytest.raises(ValueError, match=r"shape \(55,\)"):
        ragged.under_fitting_metric(nb, cadenceno=grid, cadence_mask=np.ones(54, dtype=bool))
    with pytest.raises(ValueError, match=r"remove_nans\(\)"):
        _host_batch([0, 30, 55], nan_free=False).under_fitting_metric(nb, cadenceno=grid)
    with pytest.raises(ValueError, match=r"index in \[0, 2\)"):
        ragged.under_fitting_metric(np.array([[2], [0]]), cadenceno=grid)
    with pytest.raises(ValueError, match="its own neighbour"):
        ragged.under_fitting_metric(np.array([[0], [0]]), cadenceno=grid)
    with pytest.raises(ValueError, match="neighbor_batch that carries cadence numbers"):
        ragged.under_fitting_metric(nb, cadenceno=grid, neighbor_batch=_host_batch([0, 20, 40], cadenceno=False))
    with pytest.raises(ValueError, match="at most %d" % _capi.UNDERFIT_GRID_MAX_NX):
        ragged.under_fitting_metric(nb, cadenceno=np.arange(_capi.UNDERFIT_GRID_MAX_NX + 1))
    with pytest.raises(ValueError, match="return_common goes with cadenceno"):
        ragged.under_fitting_metric(nb, return_common=True)
    with pytest.raises(ValueError, match="one cadence count"):       # without cadenceno= a ragged batch is still refused
        ragged.under_fitting_metric(nb)
    # the over-fitting metric of a ragged pair
    with pytest.raises(ValueError, match=r"offsets \(n_off\).*between 25 and 30"):
        ragged.over_fitting_metric(_host_batch([0, 30, 60]))
    with pytest.raises(ValueError, match=r"offsets \(n_off\)"):
        ragged.over_fitting_metric(_host_batch([0, 25, 55]))
    with pytest.raises(ValueError, match=r"shape \(55,\)"):
        ragged.over_fitting_metric(ragged, cadence_mask=np.ones(30, dtype=bool))
    few = np.ones(55, dtype=bool)
    few[31:] = False
    with pytest.raises(ValueError, match="target 1: .*at least three kept cadences"):
        ragged.over_fitting_metric(ragged, cadence_mask=few)
    with pytest.raises(ValueError, match="n_samples must be >= 1"):
        ragged.over_fitting_metric(ragged, n_samples=0)
    with pytest.raises(ValueError, match="regular"):
        ragged.over_fitting_metric(ragged, frequency=[0.5, 1.0, 2.5])
    # which route a mask selects: a DeviceBuffer is always the ragged mask (sum n bytes), also on a uniform batch; a host mask of
    # shape (N,) on a uniform batch is the shared one, and for B = 1, where the two shapes coincide, the uniform route is taken
    from lightkurve_amd.device import DeviceBuffer
    d_mask = DeviceBuffer.__new__(DeviceBuffer)
    d_mask.nbytes = 30
    uniform = _host_batch([0, 30, 60])
    with pytest.raises(ValueError, match="cadence_mask holds 30 bytes, the batch has 60 cadences"):
        uniform.over_fitting_metric(uniform, cadence_mask=d_mask)
    with pytest.raises(ValueError, match="at least three kept cadences"):       # (N,) on a uniform batch: the shared mask's message
        uniform.over_fitting_metric(uniform, cadence_mask=np.arange(30) < 2)
    with pytest.raises(ValueError, match="target 1: .*at least three kept cadences"):   # (sum n,): the ragged mask's
        uniform.over_fitting_metric(uniform, cadence_mask=np.arange(60) < 32)
    single = _host_batch([0, 30])
    with pytest.raises(ValueError, match="^the over-fitting metric needs at least three kept cadences"):     # B = 1: uniform route
        single.over_fitting_metric(single, cadence_mask=np.arange(30) < 2)
    # the search and the scan with cadenceno=
    cbvs = np.ones((40, 2))
    with pytest.raises(ValueError, match="target_under_score > 0 needs `neighbors`"):
        ragged.cbv_correct_optimized(cbvs, cadenceno=grid)
    with pytest.raises(ValueError, match="alpha_bounds"):
        ragged.cbv_correct_optimized(cbvs, neighbors=nb, cadenceno=grid, alpha_bounds=(10.0, 1.0))
    with pytest.raises(ValueError, match="carries cadence numbers"):
        _host_batch([0, 30, 55], cadenceno=False).cbv_correct_optimized(cbvs, neighbors=nb, cadenceno=grid)
    with pytest.raises(ValueError, match="strictly increasing"):
        ragged.cbv_correct_optimized(cbvs, neighbors=nb, cadenceno=grid[::-1].copy())
    with pytest.raises(ValueError, match=r"shape \(55,\)"):
        ragged.cbv_correct_optimized(cbvs, neighbors=nb, cadenceno=grid, cadence_mask=np.ones(40, dtype=bool))
    with pytest.raises(ValueError, match="target 1: .*at least three kept cadences"):
        ragged.cbv_correct_optimized(cbvs, neighbors=nb, cadenceno=grid, cadence_mask=few)
    with pytest.raises(ValueError, match="target 1: .*at least three kept cadences"):
        ragged.cbv_goodness_scan(cbvs, [1.0], cadenceno=grid, cadence_mask=few)
    with pytest.raises(ValueError, match="its own neighbour"):
        ragged.cbv_goodness_scan(cbvs, [1.0], neighbors=np.array([[0], [0]]), cadenceno=grid)
    with pytest.raises(ValueError, match="one cadence count"):       # without cadenceno= the search still refuses a ragged batch
        ragged.cbv_correct_optimized(np.ones((30, 2)), neighbors=nb)
    # the host-array flavours
    with pytest.raises(ValueError, match="light curve 1: every array must have its 25 cadences"):
        metrics.overfit_metric_ragged_batch([np.arange(30.0), np.arange(25.0)], [np.ones(30), np.ones(24)], [np.ones(30), np.ones(25)],
                                            [np.ones(30), np.ones(25)])
    with pytest.raises(ValueError, match="target 1: .*at least three kept cadences"):
        metrics.overfit_metric_ragged_batch([np.arange(30.0), np.arange(2.0)], [np.ones(30), np.ones(2)], [np.ones(30), np.ones(2)],
                                            [np.ones(30), np.ones(2)])
    flux = [np.ones(30), np.ones(25)]
    cad = [np.arange(100, 130), np.arange(105, 130)]
    with pytest.raises(ValueError, match="strictly increasing integer"):
        metrics.underfit_metric_ragged_batch(flux, cad, grid[::-1], nb)
    with pytest.raises(ValueError, match="light curve 1: its cadence numbers"):
        metrics.underfit_metric_ragged_batch(flux, [cad[0], cad[1][::-1]], grid, nb)
    with pytest.raises(ValueError, match="light curve 0: cadence_mask"):
        metrics.underfit_metric_ragged_batch(flux, cad, grid, nb, cadence_mask_list=[np.ones(3, dtype=bool), np.ones(25, dtype=bool)])
    with pytest.raises(ValueError, match="its own neighbour"):
        metrics.underfit_metric_ragged_batch(flux, cad, grid, np.array([[0], [0]]))
