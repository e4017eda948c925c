"""GPU: ``DeviceLightCurveBatch.fill_gaps`` (fillgaps.hip) on both paths against the numpy restatement of
tests/fillgaps_cases.py, on the batch described there (0, 1, 2, 63, 64, 65, 1500 and 5000 cadences).

Tolerances: offsets, the inserted mask, times, cadence numbers, quality, the originals' flux / flux_err and the inserted
flux_err (NaN pattern included) are exact, as is m; mu and sd agree within the project's 1e-9 relative (their sums run in the
device's tree order); an inserted flux is within 1e-9 of mu + sd * normal taken with the device's own mu and sd, and with
noise_mean = 0, noise_std = 1 the inserted fluxes ARE the normals, within the 1e-13 test_overfit_gpu.py uses for the generator
(numpy's log / cos / sin against the device's).  Every comparison prints its largest difference before it asserts
(``pytest -s``); DESIGN.md records the largest ones measured."""
import functools

import numpy as np
import pytest

import fillgaps_cases as C
import overfit_cases as OC
from lightkurve_amd import _capi, batch as lkbatch
from lightkurve_amd import device as D
from lightkurve_amd.device import DeviceLightCurveBatch
from lightkurve_amd.ingest import LightCurveBatch
from lightkurve_amd.lightcurve import LightCurve

pytestmark = pytest.mark.gpu

RTOL = 1e-9
NORMAL_ATOL = 1e-13
PATHS = ("time", "cadenceno")
ALL = tuple(range(len(C.LENGTHS)))
SEED, SID = 0x5DEECE66D1234, 5
VARIANTS = [(p, e, q) for p in PATHS for (e, q) in ((True, True), (False, False))]


def _device(lcs, path, with_err=True, with_quality=True, meta=None):
    cols, n_off = C.pack(list(lcs))
    b = DeviceLightCurveBatch.from_arrays(cols["time"], cols["flux"], cols["flux_err"] if with_err else None, n_off, meta=meta,
                                          cadenceno=cols["cadenceno"] if path == "cadenceno" else None)
    if with_quality:
        b.d_quality, k = D._upload(b.handle, cols["quality"], b.stream, np.int32)
        b._keep.append(k)
    return b


@functools.lru_cache(maxsize=None)
def dev(path, with_err=True, with_quality=True, idx=ALL):
    return _device([C.batch(path)[b] for b in idx], path, with_err, with_quality)


def _host(out, mask=None):
    r = dict(time=out.time_host(), flux=out.flux_host(), flux_err=out.flux_err_host(), quality=out.quality_host(),
             cadenceno=out.cadenceno_host(), n_off=out.n_off.copy())
    if mask is not None:
        r["inserted"] = mask.download(np.uint8, out.n_cadences, stream=out.stream).astype(bool)
    if hasattr(out, "fill_stats"):
        r["stats"] = out.fill_stats
    return r


@functools.lru_cache(maxsize=None)
def filled(path, with_err=True, with_quality=True, idx=ALL, first_target=0):
    """One fill_gaps(noise_std="std") per variant, shared by the tests; the host copies are read-only."""
    out, mask = dev(path, with_err, with_quality, idx).fill_gaps(by=path, noise_std="std", seed=SEED, first_target=first_target,
                                                                 stream_id=SID, return_mask=True)
    r = _host(out, mask)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    r["batch"], r["mask"] = out, mask
    return r


def _same(name, got, want):
    """Bitwise equality of two arrays (NaN equals NaN), the largest difference printed first."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (name, got.shape, want.shape)
    if got.dtype.kind == "f" and got.size:
        both = ~(np.isnan(got) & np.isnan(want))
        d = np.abs(got[both] - want[both])
        print("%s: max |diff| %.3g over %d values" % (name, np.nanmax(d) if d.size else 0.0, got.size))
    else:
        print("%s: %d of %d values differ" % (name, int(np.sum(got != want)), got.size))
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), name


def _rel(name, got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern" % name
    ok = ~np.isnan(want)
    r = np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)) if ok.any() else 0.0
    print("%s: max rel diff %.3g (bound %g)" % (name, r, tol))
    assert r <= tol, name


def _slices(r, b):
    return slice(int(r["n_off"][b]), int(r["n_off"][b + 1]))


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("path,with_err,with_quality", VARIANTS)
def test_exact_against_restatement(path, with_err, with_quality):
    r, exp = filled(path, with_err, with_quality), C.expected(path, with_err, with_quality)
    want_off = np.concatenate([[0], np.cumsum([e["time"].size for e in exp])])
    _same("new offsets", r["n_off"], want_off)
    cat = lambda k: np.concatenate([e[k] for e in exp])      # noqa: E731
    _same("inserted mask", r["inserted"], cat("inserted"))
    _same("time", r["time"], cat("time"))
    ins = cat("inserted")
    _same("flux of originals", r["flux"][~ins], cat("flux")[~ins])
    assert np.all(np.isfinite(r["flux"][ins]))
    if with_err:
        _same("flux_err of originals", r["flux_err"][~ins], cat("flux_err")[~ins])
        _same("flux_err of inserted cadences", r["flux_err"][ins], cat("flux_err")[ins])
        assert np.isnan(r["flux_err"][ins]).sum() == 3            # the three cadences behind the NaN error
    else:
        assert r["flux_err"] is None
    if with_quality:
        _same("quality", r["quality"], cat("quality"))
    else:
        assert r["quality"] is None
    if path == "cadenceno":
        _same("cadenceno", r["cadenceno"], cat("cadenceno"))
    else:
        assert r["cadenceno"] is None and r["batch"].d_cadenceno is None
    st = r["stats"]
    _same("m", st[:, 0], [e["m"] for e in exp])
    _rel("mu", st[:, 1], [e["mu"] for e in exp], RTOL)
    _rel("sd", st[:, 2], [e["sd"] for e in exp], RTOL)
    _same("n_inserted", st[:, 3], np.array([float(e["n_inserted"]) for e in exp]))
    nogap = C.batch(path)[4]                                          # no gap: the output equals the input
    _same("flux of the light curve without a gap", r["flux"][_slices(r, 4)], nogap["flux"])
    if path == "time":
        _same("time of the light curve without a gap", r["time"][_slices(r, 4)], nogap["time"])


@pytest.mark.parametrize("path", PATHS)
def test_inserted_flux_is_the_philox_stream(path):
    r, exp = filled(path), C.expected(path)
    first = 11
    unit, umask = dev(path).fill_gaps(by=path, noise_std=np.ones(len(ALL)), noise_mean=np.zeros(len(ALL)), seed=SEED,
                                      first_target=first, stream_id=SID, return_mask=True)
    uflux = unit.flux_host()
    _same("mask of the unit-noise run", umask.download(np.uint8, unit.n_cadences).astype(bool), r["inserted"])
    worst_rel = worst_abs = 0.0
    for b in ALL:
        s, ins = _slices(r, b), exp[b]["inserted"]
        k = int(ins.sum())
        g = OC.normals(k, 0, b, SEED, SID)
        mu, sd = r["stats"][b, 1], r["stats"][b, 2]
        got = r["flux"][s][ins]
        if k:
            worst_rel = max(worst_rel, np.max(np.abs(got - (mu + sd * g)) / np.abs(mu + sd * g)))
            worst_abs = max(worst_abs, np.max(np.abs(uflux[s][ins] - OC.normals(k, 0, first + b, SEED, SID))))
    print("inserted flux against mu + sd * normal: max rel diff %.3g (bound %g)" % (worst_rel, RTOL))
    print("unit noise against the normals: max |diff| %.3g (bound %g)" % (worst_abs, NORMAL_ATOL))
    assert worst_rel <= RTOL and worst_abs <= NORMAL_ATOL


@pytest.mark.parametrize("path", PATHS)
def test_select_gives_the_originals_back(path):
    r = filled(path)
    back = _host(r["batch"].select(r["mask"], invert=True))
    want = _host(dev(path).remove_nans())
    _same("offsets", back["n_off"], want["n_off"])
    for k in ("flux", "flux_err", "quality") + (("cadenceno",) if path == "cadenceno" else ("time",)):
        _same(k, back[k], want[k])
    if path == "cadenceno":       # originals are recomputed as (t - m c) + m c: one rounding each way
        ulp = np.max(np.abs(back["time"] - want["time"]) / np.spacing(want["time"]))
        print("recomputed original times: %.2f ulp (bound 1)" % ulp)
        assert ulp <= 1.0


@pytest.mark.parametrize("path", PATHS)
def test_bitwise_independent_of_the_batch(path):
    r = filled(path)
    keys = ("time", "flux", "flux_err", "quality", "inserted") + (("cadenceno",) if path == "cadenceno" else ())
    again, amask = dev(path).fill_gaps(by=path, noise_std="std", seed=SEED, stream_id=SID, return_mask=True)
    a = _host(again, amask)
    for k in keys + ("n_off",):
        _same("second run, " + k, a[k], r[k])
    for b in ALL:                                   # alone, first_target following the light curve
        one = filled(path, idx=(b,), first_target=b)
        for k in keys:
            assert np.array_equal(one[k], r[k][_slices(r, b)], equal_nan=True), (b, k)
        assert np.array_equal(one["stats"][0], r["stats"][b], equal_nan=True)
    perm = (7, 2, 5, 0, 6, 1, 4, 3)                # permuted: everything but the draw (its stream follows the position) permutes
    p = filled(path, idx=perm)
    for i, b in enumerate(perm):
        ins = p["inserted"][_slices(p, i)]
        for k in keys:
            got, want = p[k][_slices(p, i)], r[k][_slices(r, b)]
            if k == "flux":
                got, want = got[~ins], want[~ins]
            assert np.array_equal(got, want, equal_nan=True), (b, k)
    print("alone / permuted / second run: bitwise equal")


def test_noise_std_cdpp_and_auto():
    lcs = [C.batch("time")[b] for b in (6, 7)]
    plain = _device(lcs, "time")
    cdpp = plain.remove_nans().estimate_cdpp() * 1e-6
    assert np.all(np.isfinite(cdpp))
    by_name = plain.fill_gaps(noise_std="cdpp", seed=SEED).flux_host()
    by_array = plain.fill_gaps(noise_std=cdpp, seed=SEED).flux_host()
    _same("noise_std='cdpp' against the array", by_name, by_array)
    by_std = plain.fill_gaps(noise_std="std", seed=SEED).flux_host()
    assert not np.array_equal(by_std, by_name)
    _same("auto without NORMALIZED is std", plain.fill_gaps(seed=SEED).flux_host(), by_std)
    normed = _device(lcs, "time", meta=[{"NORMALIZED": True}, {"NORMALIZED": True}])
    _same("auto with NORMALIZED is cdpp", normed.fill_gaps(seed=SEED).flux_host(), by_name)
    half = _device(lcs, "time", meta=[{"NORMALIZED": True}, {}])
    _same("auto with one NORMALIZED is std", half.fill_gaps(seed=SEED).flux_host(), by_std)


def test_errors():
    t = np.array([0.0, 1.0, 2.0, 4.0, 3.0, 5.0, 6.0])
    f = np.ones(7)
    off = [0, 2, 7]
    with pytest.raises(ValueError, match="sorted by time"):
        DeviceLightCurveBatch.from_arrays(t, f, None, off).fill_gaps()
    with pytest.raises(ValueError, match="sorted by time: light curve 1"):
        _capi.fill_gaps_plan_batch(t, f, off)
    cad = np.array([5, 6, 10, 11, 11, 12, 13], dtype=np.int32)
    b = DeviceLightCurveBatch.from_arrays(np.arange(7.0), f, None, off, cadenceno=cad)
    with pytest.raises(ValueError, match="cadence numbers of light curve 1 are not strictly increasing"):
        b.fill_gaps()
    with pytest.raises(NotImplementedError):
        b.fill_gaps(method="linear")
    stuck = np.array([0.0, 0.0, 0.0, 1.0])       # median step 0 against a real gap: the reference's loop would never end
    with pytest.raises(ValueError, match="light curve 0"):
        DeviceLightCurveBatch.from_arrays(stuck, np.ones(4), None, [0, 4]).fill_gaps()


def test_cadence_path_makes_a_ragged_batch_uniform_for_regression_correct():
    """The use the feature exists for: two targets over the same cadence range with different cadences missing come back with
    one cadence count and go through the uniform regression_correct."""
    N, K = 300, 3
    rng = np.random.default_rng(5)
    c = np.arange(1000, 1000 + N, dtype=np.int32)
    X = np.column_stack([np.linspace(-1, 1, N), np.sin(np.linspace(0, 7, N)), np.ones(N)])
    lcs = []
    for drop in ([17, 18, 150], [40, 200, 201, 202, 298]):
        keep = np.setdiff1d(np.arange(N), drop)
        flux = 1.0 + X[:, :2] @ np.array([0.02, -0.01]) + 1e-3 * rng.standard_normal(N)
        lcs.append(dict(time=(0.02 * c)[keep], flux=flux[keep], flux_err=np.full(keep.size, 1e-3), quality=None, cadenceno=c[keep]))
    ragged = _device(lcs, "cadenceno", with_quality=False)
    with pytest.raises(ValueError, match="one cadence count"):
        ragged.regression_correct(X)
    even = ragged.fill_gaps()
    assert np.array_equal(even.n_off, [0, N, 2 * N])
    assert np.array_equal(even.cadenceno_host(), np.concatenate([c, c]))
    corrected, outl, w = even.regression_correct(X, to_host=True)
    assert corrected.shape == (2, N) and w.shape == (2, K) and np.all(np.isfinite(corrected))
    print("coefficients", w[:, :2].ravel())
    assert np.allclose(w[:, :2], [[0.02, -0.01]] * 2, atol=2e-3)


# ------------------------------------------------------------------------------------------------ host mirrors
def test_host_mirrors_return_the_device_bits():
    for path in PATHS:
        lcs = [C.batch(path)[b] for b in ALL]
        cols, n_off = C.pack(lcs)
        hb = LightCurveBatch(cols["time"], cols["flux"], cols["flux_err"], n_off)
        hb.quality = cols["quality"]
        if path == "cadenceno":
            hb.cadenceno = cols["cadenceno"]
        got, gmask = hb.fill_gaps(noise_std="std", seed=SEED, first_target=0, stream_id=SID, return_mask=True)
        r = filled(path)
        for k in ("time", "flux", "flux_err", "quality", "n_off") + (("cadenceno",) if path == "cadenceno" else ()):
            _same("LightCurveBatch.fill_gaps (%s path), %s" % (path, k), getattr(got, k), r[k])
        _same("LightCurveBatch.fill_gaps mask", gmask, r["inserted"])
    lcs = [LightCurve(time=lc["time"], flux=lc["flux"], flux_err=lc["flux_err"]) for lc in C.batch("time")]
    r = filled("time")
    fb = lkbatch.fill_gaps_batch(lcs, noise_std="std", seed=SEED, stream_id=SID)
    for k in ("time", "flux", "flux_err", "n_off"):
        _same("batch.fill_gaps_batch, " + k, getattr(fb, k), r[k])
    one = lcs[6].fill_gaps(seed=SEED)
    want = _device([C.batch("time")[6]], "time", with_quality=False).fill_gaps(seed=SEED)
    for k in ("time", "flux", "flux_err"):
        _same("LightCurve.fill_gaps, " + k, getattr(one, k), _host(want)[k])
