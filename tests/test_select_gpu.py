"""GPU: select.hip — lk_outlier_mask_batch, lk_select_columns_batch_dev, lk_cdpp_batch — and the resident methods built on
them (``outlier_mask`` / ``select`` / ``remove_outliers`` / ``estimate_cdpp`` / ``bls_search``) against the numpy restatements
of tests/select_cases.py (pinned to astropy by tests/test_select_cpu.py where astropy is importable).

TOLERANCES (set by the arithmetic, not by what the kernels give):
  * masks, selected columns, offsets: exact.  The mask inputs are checked on the CPU first: in every round of the
    restatement no finite value lies within 1e-9 std of a bound, so an ulp in the order of the std sum cannot move a cadence.
  * CDPP: rtol 1e-9, the house rule.  numpy's float64 running mean itself differs from a long-double restatement by at most
    4.2e-11 relative on these very inputs (measured on the CPU, every row and every transit_duration of the test).
  * a row alone, in the middle of a batch and in a second run: the same bits.
  * bls_search against the same loop staged through the host: exact, the same kernels see the same numbers.
"""
import functools

import numpy as np
import pytest

import select_cases as C

gpu = pytest.mark.gpu


def _dev(batch=None, with_err=True, with_quality=True):
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.ingest import LightCurveBatch
    b = C.ragged_batch() if batch is None else batch
    if not with_err:
        return DeviceLightCurveBatch.from_arrays(b["time"], b["flux"], None, b["n_off"])
    host = LightCurveBatch(b["time"], b["flux"], b["flux_err"], b["n_off"])
    if with_quality and "quality" in b:
        host.quality = b["quality"]
    return DeviceLightCurveBatch.from_batch(host)


@functools.lru_cache(maxsize=None)
def _restated(i):
    b = C.ragged_batch()
    return C.restated_mask(b["flux"], b["n_off"], **C.PARAMS[i])


def _assert_rows_equal(got, want, n_off, what):
    for r, s in enumerate(C.row_slices(n_off)):
        assert np.array_equal(got[s], want[s]), "%s: row %d (%d cadences) differs at %s" % (
            what, r, s.stop - s.start, np.flatnonzero(got[s] != want[s])[:8])


# ------------------------------------------------------------------------------------------------ outlier mask
@gpu
@pytest.mark.parametrize("i", range(len(C.PARAMS)))
def test_outlier_mask_equals_restatement(i):
    from lightkurve_amd import _capi
    b, p = C.ragged_batch(), C.PARAMS[i]
    for r, s in enumerate(C.row_slices(b["n_off"])):          # the input condition, on the CPU, before any GPU work
        assert C.clear_of_bounds(b["flux"][s], **p), "row %d has a value on a clip bound: pick another seed" % r
    want = _restated(i)
    dev = _dev()
    got = dev.outlier_mask(to_host=True, **p)
    assert got.dtype == np.bool_ and got.shape == want.shape
    _assert_rows_equal(got, want, b["n_off"], "outlier_mask(%r)" % (p,))
    d_m = dev.outlier_mask(**p)                               # resident flavour: bytes
    assert np.array_equal(d_m.download(np.uint8, dev.n_cadences, stream=dev.stream), want.astype(np.uint8))
    host = _capi.outlier_mask_batch(b["flux"], b["n_off"], **p)            # the host-pointer twin
    _assert_rows_equal(host, want, b["n_off"], "outlier_mask_batch(%r)" % (p,))
    # the asymmetric bounds select differently from the symmetric ones on these inputs
    if "sigma_lower" in p:
        assert not np.array_equal(want, _restated(0))


@gpu
def test_outlier_mask_special_rows_and_arguments():
    from lightkurve_amd import _capi
    b = C.ragged_batch()
    got = _capi.outlier_mask_batch(b["flux"], b["n_off"])
    for kind, s in zip(b["rows"], C.row_slices(b["n_off"])):
        if kind == "all-nan":
            assert got[s].all()
        if kind == "constant":
            assert not got[s].any()
    assert np.array_equal(got, ~np.isfinite(b["flux"]) | _restated(0))
    assert np.array_equal(_capi.outlier_mask_batch(b["flux"], b["n_off"], maxiters=0), ~np.isfinite(b["flux"]))
    assert _capi.outlier_mask_batch(np.zeros(0), [0]).shape == (0,)
    assert _capi.outlier_mask_batch(np.zeros(0), [0, 0, 0]).shape == (0,)
    with pytest.raises(ValueError):
        _capi.outlier_mask_batch(b["flux"], b["n_off"], maxiters=-2)
    with pytest.raises(ValueError):
        _capi.outlier_mask_batch(b["flux"], b["n_off"], sigma_upper=float("nan"))


# ------------------------------------------------------------------------------------------------ select
def _check_select(out, b, keep, with_err=True, with_quality=True):
    want_off = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[b["n_off"]]
    assert np.array_equal(out.n_off, want_off)
    assert out.n_cadences == int(keep.sum())
    assert np.array_equal(out.time_host(), b["time"][keep])
    assert np.array_equal(out.flux_host().view(np.uint64), b["flux"][keep].view(np.uint64))       # NaN payloads included
    if with_err:
        assert np.array_equal(out.flux_err_host(), b["flux_err"][keep])
    else:
        assert out.d_flux_err is None
    if with_quality:
        assert np.array_equal(out.quality_host(), b["quality"][keep])
    else:
        assert out.d_quality is None


@gpu
def test_select_equals_boolean_indexing():
    b = C.ragged_batch()
    dev = _dev()
    dev.meta[1]["LABEL"] = "kept"
    rng = np.random.default_rng(5)
    mask = rng.random(dev.n_cadences) < 0.6
    out = dev.select(mask)                                             # host bool mask
    _check_select(out, b, mask)
    assert out.meta[1]["LABEL"] == "kept" and out.meta is not dev.meta
    assert out.is_sorted == dev.is_sorted and out.nan_free == dev.nan_free and out.median_flux is None
    _check_select(dev.select(mask.astype(np.uint8) * 7), b, mask)      # host uint8 mask: any non-zero byte keeps
    _check_select(dev.select(mask, invert=True), b, ~mask)
    d_m = dev.outlier_mask()                                           # DeviceBuffer mask
    _check_select(dev.select(d_m), b, _restated(0))
    _check_select(dev.select(d_m, invert=True), b, ~_restated(0))
    ones = np.ones(dev.n_cadences, dtype=bool)
    _check_select(dev.select(ones), b, ones)
    empty = dev.select(~ones)                                          # every row empty
    _check_select(empty, b, ~ones)
    assert not empty.n_off.any()
    _check_select(empty.select(np.zeros(0, dtype=bool)), b, ~ones)     # and a batch without cadences selects to itself
    normalized = dev.normalize()
    assert normalized.median_flux is not None and normalized.select(np.ones(normalized.n_cadences, dtype=bool)).median_flux is None


@gpu
def test_select_without_flux_err_or_quality():
    b = C.ragged_batch()
    dev = _dev(with_err=False)
    mask = np.arange(dev.n_cadences) % 3 != 1
    _check_select(dev.select(mask), b, mask, with_err=False, with_quality=False)
    _check_select(_dev(with_quality=False).select(mask, invert=True), b, ~mask, with_quality=False)


@gpu
def test_select_rejects_bad_masks_and_aliasing():
    import ctypes
    from lightkurve_amd import _capi
    from lightkurve_amd.device import DeviceBuffer
    dev = _dev()
    n = dev.n_cadences
    with pytest.raises(ValueError):
        dev.select(np.ones(n - 1, dtype=bool))
    with pytest.raises(ValueError):
        dev.select(np.ones((n, 1), dtype=bool))
    with pytest.raises(ValueError):
        dev.select(np.ones(n, dtype=np.float64))
    with pytest.raises(ValueError):
        dev.select(DeviceBuffer(dev.handle, n + 3))
    # the C entry point refuses an output that is (or overlaps) an input
    vp = ctypes.c_void_p
    d_m = dev.outlier_mask()
    B = len(dev)
    new_off = np.zeros(B + 1, dtype=np.int64)
    elem = np.array([8], dtype=np.int32)
    for out_ptr in (dev.d_flux.ptr, dev.d_flux.ptr + 64):
        cin, cout = (vp * 1)(dev.d_flux.ptr), (vp * 1)(out_ptr)
        rc = _capi._lib.lk_select_columns_batch_dev(dev.handle._h, B, dev.n_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                    vp(d_m.ptr), 0, 1, elem.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cin, cout,
                                                    new_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None)
        assert rc == _capi.LK_EINVAL
    assert np.array_equal(dev.flux_host().view(np.uint64), C.ragged_batch()["flux"].view(np.uint64))      # untouched


# ------------------------------------------------------------------------------------------------ remove_outliers
@gpu
def test_remove_outliers_equals_lightcurve_remove_outliers():
    from lightkurve_amd.lightcurve import LightCurve
    b = C.ragged_batch()
    dev = _dev()
    out, d_m = dev.remove_outliers(return_mask=True)
    mask = d_m.download(np.uint8, dev.n_cadences, stream=dev.stream).astype(bool)
    assert out.nan_free
    host = out.to_host()
    for r, s in enumerate(C.row_slices(b["n_off"])):
        lc = LightCurve(time=b["time"][s], flux=b["flux"][s], flux_err=b["flux_err"][s])
        clean, m = lc.remove_outliers(return_mask=True)           # the symmetric path of the parent commit: the yardstick
        assert np.array_equal(mask[s], m), "row %d" % r
        got = host[r]
        assert np.array_equal(got.time, clean.time) and np.array_equal(got.flux, clean.flux)
        assert np.array_equal(got.flux_err, clean.flux_err)
    assert np.array_equal(host.quality, b["quality"][~mask])
    assert np.array_equal(dev.remove_outliers().flux_host(), host.flux)


@gpu
def test_lightcurve_remove_outliers_keeps_its_values_and_gains_bounds():
    from lightkurve_amd import _capi
    from lightkurve_amd.ingest import LightCurveBatch
    from lightkurve_amd.lightcurve import LightCurve
    from oracle import np_oracle as O
    b = C.ragged_batch()
    rows = C.row_slices(b["n_off"])
    for r in (0, 7, 9, 11):                                       # 1023, 65 (NaN), 1025 (+inf), 4500 (NaN) cadences
        s = rows[r]
        lc = LightCurve(time=b["time"][s], flux=b["flux"][s], flux_err=b["flux_err"][s])
        for sigma in (5.0, 3.0):
            direct = _capi.sigma_clip_batch(b["flux"][s], [0, s.stop - s.start], sigma=sigma, maxiters=5)
            clean, m = lc.remove_outliers(sigma=sigma, return_mask=True)
            assert np.array_equal(m, direct) and np.array_equal(m, O.sigma_clip_mask(b["flux"][s], sigma=sigma))
            assert np.array_equal(clean.flux, b["flux"][s][~direct])
        for p in C.PARAMS[1:]:                                    # the new arguments go through lk_outlier_mask_batch
            clean, m = lc.remove_outliers(return_mask=True, **p)
            assert np.array_equal(m, C.sigma_clip_mask_asym(b["flux"][s], **p))
            assert np.array_equal(clean.time, b["time"][s][~m])
    # the clipped cadences of the first row at the default arguments, from the restatement
    first = LightCurve(flux=b["flux"][rows[0]]).remove_outliers(return_mask=True)[1]
    assert np.array_equal(np.flatnonzero(first), np.flatnonzero(_restated(0)[rows[0]])) and first.sum() == 18
    host = LightCurveBatch(b["time"], b["flux"], b["flux_err"], b["n_off"])
    host.quality = b["quality"]
    p = C.PARAMS[1]
    out, m = host.remove_outliers(return_mask=True, **p)
    assert np.array_equal(m, _restated(1))
    assert np.array_equal(out.flux, b["flux"][~m]) and np.array_equal(out.quality, b["quality"][~m])
    assert np.array_equal(out.n_off, np.concatenate([[0], np.cumsum(~m)])[b["n_off"]])


# ------------------------------------------------------------------------------------------------ CDPP
@gpu
@pytest.mark.parametrize("td", C.DURATIONS)
def test_cdpp_batch_equals_numpy_tail(td):
    from lightkurve_amd import _capi
    b = C.ragged_batch()
    outl = _restated(0)
    got = _capi.cdpp_batch(b["flux"], b["n_off"], outlier=outl, transit_duration=td)
    want = np.array([C.cdpp_tail(b["flux"][s], outl[s], td) for s in C.row_slices(b["n_off"])])
    print("transit_duration %d: got %r\nwant %r" % (td, got, want))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want).sum() == 3                               # the two empty rows and the all-NaN one
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0.0)
    # no mask: every cadence counts (rows without a non-finite value only)
    fin = [s for s in C.row_slices(b["n_off"]) if s.stop > s.start and np.all(np.isfinite(b["flux"][s]))]
    flat = np.concatenate([b["flux"][s] for s in fin])
    off = np.concatenate([[0], np.cumsum([s.stop - s.start for s in fin])])
    got = _capi.cdpp_batch(flat, off, transit_duration=td)
    want = np.array([C.cdpp_tail(b["flux"][s], None, td) for s in fin])
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0.0)


@gpu
def test_cdpp_bits_do_not_depend_on_batch_position_or_run():
    from lightkurve_amd import _capi
    b = C.ragged_batch()
    outl = _restated(0)
    whole = _capi.cdpp_batch(b["flux"], b["n_off"], outlier=outl, transit_duration=13)
    again = _capi.cdpp_batch(b["flux"], b["n_off"], outlier=outl, transit_duration=13)
    assert np.array_equal(whole.view(np.uint64), again.view(np.uint64))
    for r in (0, 10, 11):                                          # 1023, 2049 and 4500 cadences, all inside the batch
        s = C.row_slices(b["n_off"])[r]
        alone = _capi.cdpp_batch(b["flux"][s], [0, s.stop - s.start], outlier=outl[s], transit_duration=13)
        assert np.array_equal(alone, whole[r:r + 1])
    with pytest.raises(ValueError):
        _capi.cdpp_batch(b["flux"], b["n_off"], transit_duration=0)
    with pytest.raises(ValueError):
        _capi.cdpp_batch(b["flux"], b["n_off"], transit_duration=13.0)


@functools.lru_cache(maxsize=None)
def _cdpp_curves():
    from lightkurve_amd.lightcurve import LightCurve
    rng = np.random.default_rng(C.SEED + 2)
    lcs = []
    for k, n in enumerate((900, 1301, 1777, 2048, 2333, 2600)):
        t = 1500.0 + 0.0204 * np.arange(n)
        f = (1.0 + 2e-3 * np.sin(2 * np.pi * t / 7.3 + k) + 3e-4 * rng.standard_normal(n)) * (1000.0 + 50 * k)
        f[rng.random(n) < 0.004] *= 1.01
        if k % 2:
            f[rng.choice(n, 5, replace=False)] = np.nan
        lcs.append(LightCurve(time=t, flux=f, flux_err=np.full(n, 0.3)))
    return tuple(lcs)


@gpu
@pytest.mark.parametrize("kw", [dict(), dict(transit_duration=7, savgol_window=51, sigma=4)])
def test_estimate_cdpp_equals_host_list_route(kw):
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.lightcurve import estimate_cdpp_batch
    lcs = list(_cdpp_curves())
    want = estimate_cdpp_batch(lcs, **kw)
    dev = DeviceLightCurveBatch.from_lightcurves(lcs)
    got = dev.estimate_cdpp(**kw)
    print("estimate_cdpp(%r): got %r want %r" % (kw, got, want))
    assert got.shape == (len(lcs),) and np.all(np.isfinite(want)) and np.all(want > 50)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0.0)
    assert np.array_equal(got, dev.estimate_cdpp(**kw))


@gpu
def test_estimate_cdpp_argument_errors():
    from lightkurve_amd.device import DeviceLightCurveBatch
    lcs = list(_cdpp_curves())[:2]
    dev = DeviceLightCurveBatch.from_lightcurves(lcs)
    with pytest.raises(ValueError, match="transit_duration must be an integer"):
        dev.estimate_cdpp(transit_duration=6.5)
    t = lcs[0].time.copy()
    t[[3, 4]] = t[[4, 3]]
    unsorted = DeviceLightCurveBatch.from_arrays(t, lcs[0].flux, lcs[0].flux_err, [0, len(t)])
    with pytest.raises(ValueError, match="sorted"):
        unsorted.estimate_cdpp()


# ------------------------------------------------------------------------------------------------ bls_search
@gpu
def test_bls_search_equals_the_loop_staged_through_the_host():
    from lightkurve_amd.device import DeviceLightCurveBatch
    f = C.bls_field()
    step = float(C.BLS_GRID[1] - C.BLS_GRID[0])
    # on the CPU first: the BLS oracle finds the two injected signals, the deeper one first, in every light curve
    for s in C.row_slices(f["n_off"]):
        found = C.bls_search_oracle(f["time"][s], f["flux"][s], f["flux_err"][s])
        assert C.near_harmonic(found[0][0], C.BLS_PERIODS[0], step) and C.near_harmonic(found[1][0], C.BLS_PERIODS[1], step)
    dev = DeviceLightCurveBatch.from_arrays(f["time"], f["flux"], f["flux_err"], f["n_off"])
    signals, residual = dev.bls_search(C.BLS_GRID, n_signals=2, duration=C.BLS_DURATIONS)
    # the same loop with every batch taken through the host
    cur, staged = dev, []
    for _ in range(2):
        res = cur.bls(C.BLS_GRID, duration=C.BLS_DURATIONS)
        pk = res.peaks()
        mask = res.transit_mask(pk["period"], pk["duration"], pk["transit_time"], to_host=True)
        host = res._batch.to_host()                # the NaN-free batch the search ran on: what the mask refers to
        keep = ~mask
        off = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[host.n_off]
        cur = DeviceLightCurveBatch.from_arrays(host.time[keep], host.flux[keep], host.flux_err[keep], off)
        staged.append(pk)
    assert len(signals) == 2
    for got, want in zip(signals, staged):
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    want_res, got_res = cur.to_host(), residual.to_host()
    assert np.array_equal(got_res.n_off, want_res.n_off) and got_res.n_off[-1] < f["n_off"][-1]
    for col in ("time", "flux", "flux_err"):
        assert np.array_equal(getattr(got_res, col), getattr(want_res, col)), col
    for b in range(4):
        assert C.near_harmonic(signals[0]["period"][b], C.BLS_PERIODS[0], step)
        assert C.near_harmonic(signals[1]["period"][b], C.BLS_PERIODS[1], step)


@gpu
def test_bls_search_raises_for_a_light_curve_without_cadences():
    """A light curve with no cadence left makes the next round's ``bls`` raise.  (A light curve cannot be made to lose its
    last cadences to its OWN best box in a way that survives rounding: the box that covers every cadence starts at the
    first one, which then sits exactly on the window's edge.  The empty light curve comes from ``select`` here.)"""
    from lightkurve_amd.device import DeviceLightCurveBatch
    f = C.bls_field()
    dev = DeviceLightCurveBatch.from_arrays(f["time"], f["flux"], f["flux_err"], f["n_off"])
    drop = np.zeros(dev.n_cadences, dtype=bool)
    drop[int(f["n_off"][2]):int(f["n_off"][3])] = True            # light curve 2 loses every cadence
    emptied = dev.select(drop, invert=True)
    assert emptied.n_off[3] == emptied.n_off[2]
    with pytest.raises(ValueError, match="no finite flux"):
        emptied.bls_search(C.BLS_GRID, n_signals=2, duration=C.BLS_DURATIONS)
    flux = f["flux"].copy()
    flux[int(f["n_off"][1]):int(f["n_off"][2])] = np.nan           # or loses them to remove_nans inside the first round
    with pytest.raises(ValueError, match="no finite flux"):
        DeviceLightCurveBatch.from_arrays(f["time"], flux, f["flux_err"], f["n_off"]).bls_search(
            C.BLS_GRID, n_signals=2, duration=C.BLS_DURATIONS)
    with pytest.raises(ValueError):
        dev.bls_search(C.BLS_GRID, n_signals=0)
