"""GPU: SFFCorrector for a resident batch (csrc/sff.hip) and the moment centroids of a resident cube batch, against the numpy /
scipy reference of tests/sff_cases.py.

Tolerances: arclength, design matrix, priors and knots 1e-12 (relative to values of order one; the kernels and numpy differ by
a few roundings); corrected flux, ``spline`` and ``sff`` 1e-9 of the flux level (the house rule); outlier masks identical
(test_sff_cpu.py checks that no reference residual sits near the 5-sigma decision).  Coefficients are never compared: the
normal matrix is ill-conditioned and only models are comparable (test_sff_cpu.py).
"""
import ctypes
import functools

import numpy as np
import pytest

import sff_cases as C
from lightkurve_amd import _capi
from lightkurve_amd.correctors import SFFCorrector, sff_correct_batch
from lightkurve_amd.device import DeviceBuffer, DeviceLightCurveBatch, DevicePixelCubeBatch
from lightkurve_amd.lightcurve import LightCurve

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)


def device_batch(targets):
    return DeviceLightCurveBatch.from_arrays(C.pack(targets, "time"), C.pack(targets, "flux"), C.pack(targets, "flux_err"),
                                             C.offsets(targets))


def run(targets, wps, **kw):
    """sff_correct of a list of target dicts on the device -> host dict."""
    b = device_batch(targets)
    return b.sff_correct(C.pack(targets, "col"), C.pack(targets, "row"), window_points=wps, bins=C.BINS, degree=C.DEGREE,
                         timescale=C.TIMESCALE, to_host=True, **kw)


@functools.lru_cache(maxsize=None)
def batch_result():
    """The batch of sff_cases.batch() (three targets + the too-short one) corrected once; shared, read-only."""
    targets, wps = C.batch()
    return run(targets, wps)


def rows(res, key, index):
    off = C.offsets(C.batch()[0])
    return res[key][off[index]:off[index + 1]]


def check_against_reference(dev, ref, what):
    for key, level in (("flux", C.LEVEL), ("flux_err", C.LEVEL), ("spline", 1.0), ("sff", 1.0)):
        err = np.max(np.abs(dev[key] - ref[key])) / level
        print("%s %s: max |device - reference| / level = %.3g" % (what, key, err))
        assert err < 1e-9, (what, key, err)
    assert np.array_equal(dev["outlier_mask"], ref["outlier_mask"]), what


# ------------------------------------------------------------------------------------------------ arclength
def test_arclength_matches_numpy_and_flips_alike():
    targets, _ = C.batch()
    arc, flipped = _capi.sff_arclength_batch(C.pack(targets, "col"), C.pack(targets, "row"), C.offsets(targets))
    off = C.offsets(targets)
    flips = []
    for b, t in enumerate(targets):
        ref, flip = C.arclength(t["col"], t["row"])
        flips.append(flip)
        err = np.max(np.abs(arc[off[b]:off[b + 1]] - ref)) / np.max(ref)
        print("target %d: arclength max rel err %.3g, flip %s" % (b, err, flip))
        assert err < 1e-12
    assert list(flipped) == flips and flips[:3] == [False, True, False]
    # the resident call gives the same bits, and so does the arclength sff_correct reports
    dev = device_batch(targets).sff_arclength(C.pack(targets, "col"), C.pack(targets, "row"))
    assert np.array_equal(dev, arc)
    assert np.array_equal(batch_result()["arclength"], arc)


# ------------------------------------------------------------------------------------------------ design matrix
def design_on_device(indices):
    """lk_sff_design_batch_dev for the targets `indices` of the batch (one group) -> host arrays."""
    targets, wps = C.batch()
    ts = [targets[i] for i in indices]
    b = device_batch(ts)
    h, n, B = b.handle, b.n_cadences, len(ts)
    arc = b.sff_arclength(C.pack(ts, "col"), C.pack(ts, "row"))
    d_arc = DeviceBuffer(h, n * 8)
    d_arc.upload(arc)
    win_off, wp = _capi.sff_window_arrays([wps[i] for i in indices], b.n_off)
    nk = C.n_knots_of(ts[0]["time"])
    W = len(wps[indices[0]]) + 1
    K = nk + W * (C.BINS + C.DEGREE)
    sizes = dict(X=n * K, mu=B * K, sg=B * K, kt=B * (nk - 2), kw=B * W * (C.BINS + 1), f=n, e=n)
    bufs = {k: DeviceBuffer(h, v * 8) for k, v in sizes.items()}
    _capi._check(_capi._lib.lk_sff_design_batch_dev(
        h._h, B, b.n_off.ctypes.data_as(_i64p), _vp(b.d_time.ptr), _vp(b.d_flux.ptr), _vp(b.d_flux_err.ptr), _vp(d_arc.ptr),
        win_off.ctypes.data_as(_i32p), wp.ctypes.data_as(_i32p), C.BINS, C.DEGREE, nk, *[_vp(bufs[k].ptr) for k in sizes], None))
    out = {k: bufs[k].download(np.float64, sizes[k]) for k in sizes}
    out.update(X=out["X"].reshape(n, K), mu=out["mu"].reshape(B, K), sg=out["sg"].reshape(B, K), kt=out["kt"].reshape(B, nk - 2),
               kw=out["kw"].reshape(B, W, C.BINS + 1), arc=arc, n_off=b.n_off, nk=nk, W=W)
    return out


@pytest.mark.parametrize("indices", [(0, 2), (1,)])
def test_design_matrix_matches_reference_and_the_spline_kernel(indices):
    targets, wps = C.batch()
    d = design_on_device(list(indices))
    nbw = C.BINS + C.DEGREE
    for g, i in enumerate(indices):
        ref = C.reference(i)
        t = targets[i]
        N = len(t["time"])
        X = d["X"][d["n_off"][g]:d["n_off"][g + 1]]
        assert X.shape == ref["X"].shape
        figs = dict(X=np.max(np.abs(X - ref["X"])), prior_mu=np.max(np.abs(d["mu"][g] - ref["prior_mu"])),
                    prior_sigma=np.max(np.abs(d["sg"][g] / ref["prior_sigma"] - 1)),
                    knots_time=np.max(np.abs(d["kt"][g] / ref["knots_time"] - 1)),
                    knots_win=np.max(np.abs(d["kw"][g] - ref["knots_win"])),
                    f=np.max(np.abs(d["f"][d["n_off"][g]:d["n_off"][g + 1]] - ref["f"])))
        print("target %d:" % i, {k: "%.3g" % v for k, v in figs.items()})
        for k, v in figs.items():
            assert v < 1e-12, (i, k, v)
        # every block has the bits lk_spline_basis_batch gives for the same x and the knots the device chose
        arc = d["arc"][d["n_off"][g]:d["n_off"][g + 1]]
        assert np.array_equal(X[:, :d["nk"]], _capi.spline_basis_batch(t["time"][None], d["kt"][g][None], degree=3)[0])
        lo, up = np.append(0, wps[i]), np.append(wps[i], N)
        for j in range(d["W"]):
            x = np.full(N, -1.0)
            x[lo[j]:up[j]] = arc[lo[j]:up[j]]
            blk = X[:, d["nk"] + j * nbw:d["nk"] + (j + 1) * nbw]
            assert np.array_equal(blk, _capi.spline_basis_batch(x[None], d["kw"][g, j][None], degree=C.DEGREE)[0]), (i, j)
            outside = np.ones(N, bool)
            outside[lo[j]:up[j]] = False
            # outside the window: [1, 0, ..., 0], the 1 as the basis itself rounds it at its lower boundary knot (the bitwise
            # check above holds for these rows too), one value for all of them
            assert np.all(np.abs(blk[outside, 0] - 1.0) < 1e-12) and np.all(blk[outside, 1:] == 0.0)
            assert np.unique(blk[outside, 0]).size <= 1


# ------------------------------------------------------------------------------------------------ the correction
def test_correct_matches_reference_masks_and_statuses():
    res = batch_result()
    assert list(res["status"]) == [0, 0, 0, 1]
    for i in range(3):
        dev = {k: rows(res, k, i) for k in ("flux", "flux_err", "spline", "sff", "outlier_mask")}
        check_against_reference(dev, C.reference(i), "target %d" % i)
        assert np.all(dev["outlier_mask"][C.batch()[0][i]["spikes"]])
    for k in ("flux", "flux_err", "spline", "sff"):                  # the too-short target: NaN, no outlier, no exception
        assert np.all(np.isnan(rows(res, k, 3)))
    assert not rows(res, "outlier_mask", 3).any()


def test_restore_trend():
    targets, wps = C.batch()
    dev = run(targets[:1], wps[:1], restore_trend=True)
    check_against_reference(dev, C.reference(0, restore_trend=True), "restore_trend")
    plain = rows(batch_result(), "flux", 0)
    assert np.max(np.abs(dev["flux"] - plain)) > 1e-4 * C.LEVEL       # the slow sine is back


def test_cadence_mask():
    targets, wps = C.batch()
    dev = run(targets[:1], wps[:1], cadence_mask=C.cadence_mask(0))
    check_against_reference(dev, C.reference(0, masked=True), "cadence_mask")
    assert not np.array_equal(dev["flux"], rows(batch_result(), "flux", 0))


def test_one_window():
    targets, _ = C.batch()
    wp = [C.even_points(len(targets[2]["time"]), 1)]
    assert wp[0].size == 0
    dev = run(targets[2:3], wp)
    assert list(dev["status"]) == [0]
    check_against_reference(dev, C.reference(2, windows=1), "windows=1")


def test_non_finite_input_is_a_status():
    targets, wps = C.batch()
    bad = dict(targets[1])
    bad["col"] = bad["col"].copy()
    bad["col"][17] = np.nan
    dev = run([targets[0], bad], wps[:2])
    assert list(dev["status"]) == [0, 2]
    off = C.offsets([targets[0], bad])
    assert np.array_equal(dev["flux"][:off[1]], rows(batch_result(), "flux", 0))
    assert np.all(np.isnan(dev["flux"][off[1]:]))


# ------------------------------------------------------------------------------------------------ bitwise properties
KEYS = ("flux", "flux_err", "spline", "sff", "outlier_mask", "arclength")


def test_two_runs_agree_bitwise():
    targets, wps = C.batch()
    again = run(targets, wps)
    for k in KEYS:
        assert np.array_equal(again[k], batch_result()[k], equal_nan=True), k


def test_target_alone_equals_target_in_batch():
    targets, wps = C.batch()
    for i in (0, 1, 2):
        alone = run(targets[i:i + 1], wps[i:i + 1])
        for k in KEYS:
            assert np.array_equal(alone[k], rows(batch_result(), k, i)), (i, k)


def test_one_target_per_chunk_equals_one_chunk():
    targets, wps = C.batch()
    n_off = C.offsets(targets)
    nk = _capi.sff_n_knots([t["time"][0] for t in targets], [t["time"][-1] for t in targets], C.TIMESCALE)
    win_off, _ = _capi.sff_window_arrays(wps, n_off)
    budget = 300000                                   # below the two targets of the (8, 4) group together, above either alone
    assert _capi.sff_scratch_bytes(n_off, nk, win_off, C.BINS, C.DEGREE)[1] == 2
    assert _capi.sff_scratch_bytes(n_off, nk, win_off, C.BINS, C.DEGREE, budget)[1] == 3
    small = run(targets, wps, max_scratch_bytes=budget)
    for k in KEYS:
        assert np.array_equal(small[k], batch_result()[k], equal_nan=True), k
    with pytest.raises(ValueError):
        run(targets, wps, max_scratch_bytes=100000)


def test_host_api_gives_the_same_bits():
    """SFFCorrector / sff_correct_batch (host light curves, staged through lk_sff_correct_batch) = the resident call."""
    targets, wps = C.batch()
    lcs = [LightCurve(time=t["time"], flux=t["flux"], flux_err=t["flux_err"]) for t in targets[:3]]
    out, info = sff_correct_batch(lcs, [t["col"] for t in targets[:3]], [t["row"] for t in targets[:3]], window_points=wps[:3],
                                  bins=C.BINS, degree=C.DEGREE, timescale=C.TIMESCALE)
    for i in range(3):
        assert np.array_equal(out[i].flux, rows(batch_result(), "flux", i))
        assert np.array_equal(info["sff"][i], rows(batch_result(), "sff", i))
    corr = SFFCorrector(lcs[1])
    lc = corr.correct(targets[1]["col"], targets[1]["row"], window_points=wps[1], bins=C.BINS, degree=C.DEGREE, timescale=C.TIMESCALE)
    assert np.array_equal(lc.flux, rows(batch_result(), "flux", 1))
    assert np.array_equal(corr.diagnostic_lightcurves["spline"].flux, rows(batch_result(), "spline", 1))
    assert np.array_equal(corr.outlier_mask, rows(batch_result(), "outlier_mask", 1))
    assert np.array_equal(corr.window_points, wps[1]) and corr.arclength.shape == lc.flux.shape
    # the automatic windows: the arclength comes back, sff_window_points runs on the host, the correction still removes the roll
    auto = SFFCorrector(lcs[0]).correct(targets[0]["col"], targets[0]["row"], windows=4, bins=C.BINS, timescale=C.TIMESCALE)
    assert np.std(auto.flux / C.LEVEL) < np.std(targets[0]["flux"] / C.LEVEL)


# ------------------------------------------------------------------------------------------------ centroids
def centroid_reference(flux, mask, column, row):
    ny, nx = flux.shape[-2:]
    yy, xx = np.indices((ny, nx))
    f = np.where(mask, flux.astype(np.float64), np.nan)
    with np.errstate(all="ignore"):
        tot = np.nansum(f, axis=(-2, -1))
        col = np.nansum((column + xx) * f, axis=(-2, -1)) / tot
        rw = np.nansum((row + yy) * f, axis=(-2, -1)) / tot
    return col, rw


def test_estimate_centroids():
    rng = np.random.RandomState(21)
    B, N, ny, nx = 2, 64, 11, 11
    yy, xx = np.indices((ny, nx))
    cx = 5.0 + 0.8 * rng.rand(B, N, 1, 1)
    cy = 5.2 + 0.8 * rng.rand(B, N, 1, 1)
    flux = (500.0 * np.exp(-0.5 * ((xx - cx) ** 2 + (yy - cy) ** 2) / 1.5 ** 2) + rng.rand(B, N, ny, nx)).astype(np.float32)
    flux[rng.rand(B, N, ny, nx) < 0.02] = np.nan
    flux[1, 40] = np.nan                                            # an all-NaN cadence
    mask = np.zeros((B, ny, nx), bool)
    mask[0, 2:9, 2:9] = True
    mask[1, 1:8, 3:10] = True                                       # one mask per cutout
    t = np.tile(np.arange(N) * C.CADENCE, (B, 1))
    cubes = DevicePixelCubeBatch.from_arrays(t, flux, np.ones_like(flux))
    col, row = cubes.estimate_centroids(aperture_mask=mask, column=5, row=7, to_host=True)
    rc, rr = centroid_reference(flux, mask[:, None], 5, 7)
    assert np.isnan(col[1, 40]) and np.isnan(row[1, 40]) and np.isnan(rc[1, 40])
    ok = ~np.isnan(rc)
    assert ok.sum() == B * N - 1
    err = max(np.max(np.abs(col[ok] / rc[ok] - 1)), np.max(np.abs(row[ok] / rr[ok] - 1)))
    print("centroids: max rel err %.3g" % err)
    assert err < 1e-12
    shared = cubes.estimate_centroids(aperture_mask=mask[0], column=5, row=7, to_host=True)     # one mask for the batch
    assert np.array_equal(shared[0][0], col[0]) and np.array_equal(shared[1][0], row[0])


# ------------------------------------------------------------------------------------------------ the resident K2 chain
def test_cube_to_periodogram_chain_equals_the_staged_host_chain():
    targets, wps = C.batch()
    ts = [targets[0], C.make_target(31, 600)]
    wp = [wps[0], wps[0]]
    ny = nx = 11
    yy, xx = np.indices((ny, nx))
    flux = np.stack([(t["flux"][:, None, None] / (2 * np.pi * 1.2 ** 2)
                      * np.exp(-0.5 * ((xx - (t["col"][:, None, None] - 5.0)) ** 2 + (yy - (t["row"][:, None, None] - 15.0)) ** 2)
                               / 1.2 ** 2)) for t in ts]).astype(np.float32)
    err = np.full_like(flux, 0.05)
    cubes = DevicePixelCubeBatch.from_arrays(np.stack([t["time"] for t in ts]), flux, err)
    lcs = cubes.to_lightcurves()
    d_col, d_row = cubes.estimate_centroids(column=5, row=15)
    res = lcs.sff_correct(d_col, d_row, window_points=wp, bins=C.BINS, degree=C.DEGREE, timescale=C.TIMESCALE, to_host=False)
    assert list(res["status"]) == [0, 0]
    freq = np.linspace(0.05, 6.0, 400)
    peaks = res["lc"].to_periodogram_peaks(freq)
    # the staged route: everything back on the host between the stages
    hb = lcs.to_host()
    col, row = cubes.estimate_centroids(column=5, row=15, to_host=True)
    host = _capi.sff_correct_batch(hb.time, hb.flux, hb.flux_err, col.ravel(), row.ravel(), hb.n_off, wp, bins=C.BINS,
                                   degree=C.DEGREE, timescale=C.TIMESCALE)
    assert np.array_equal(res["lc"].flux_host(), host["flux"]) and np.array_equal(res["lc"].flux_err_host(), host["flux_err"])
    staged = DeviceLightCurveBatch.from_arrays(hb.time, host["flux"], host["flux_err"], hb.n_off).to_periodogram_peaks(freq)
    assert np.array_equal(peaks, staged)
    # and the correction did its job: the 12-cadence roll no longer dominates the light curve
    raw = hb.flux[:600] / np.median(hb.flux[:600])
    fixed = host["flux"][:600] / np.median(host["flux"][:600])
    mad = lambda v: np.median(np.abs(v - np.median(v)))                                         # noqa: E731 (the spikes stay)
    assert mad(fixed) < 0.5 * mad(raw)
