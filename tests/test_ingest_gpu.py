"""GPU parity: batch ingest — remove_nans + normalize, create_transit_mask, bin — for a ragged batch
in one launch each, against golden vectors from the reference (lightkurve; bin through astropy 4.3.1's
aggregate_downsample the way lightkurve calls it) and the numpy oracle.  Tolerances (stated): kept times identical,
normalised flux / errors 1e-15 relative (one division by the same median), transit masks identical, binned flux 1e-13
and errors 1e-12 relative (the reference sums each bin pairwise, the kernel sequentially), bin times 1e-9 d."""
import numpy as np
import pytest

from lightkurve_amd import LightCurve, LightCurveBatch
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu


def _null_args(monkeypatch, entry, *positions):
    """Make the _capi wrapper's call of the C entry point `entry` pass NULL at argument `positions`: the optional outputs
    the wrapper always asks for."""
    from lightkurve_amd import _capi
    real = getattr(_capi.load_library(), entry)
    monkeypatch.setattr(_capi._lib, entry, lambda *a: real(*[None if i in positions else x for i, x in enumerate(a)]))


def _batch(g):
    n = int(g["n"])
    return LightCurveBatch.from_lightcurves([LightCurve(time=g["time_%d" % b], flux=g["flux_%d" % b], flux_err=g["err_%d" % b])
                                             for b in range(n)]), n


def test_remove_nans_normalize_batch_vs_reference(golden, monkeypatch):
    from lightkurve_amd import _capi
    g = golden("ingest")
    batch, n = _batch(g)
    clean = batch.remove_nans()
    norm = batch.normalize()
    for b in range(n):
        assert np.array_equal(clean[b].time, g["clean_time_%d" % b])
        assert np.array_equal(clean[b].flux, g["flux_%d" % b][~np.isnan(g["flux_%d" % b])])
        assert np.array_equal(norm[b].time, g["clean_time_%d" % b])
        assert np.allclose(norm[b].flux, g["clean_flux_%d" % b], rtol=1e-15, atol=0)
        assert np.allclose(norm[b].flux_err, g["clean_err_%d" % b], rtol=1e-15, atol=0, equal_nan=True)
        assert norm.median_flux[b] == np.nanmedian(g["flux_%d" % b])
        assert norm.meta[b]["NORMALIZED"] is True
    # median_out NULL: the same cadences, flux and errors
    ref = _capi.ingest_batch(batch.time, batch.flux, batch.n_off, flux_err=batch.flux_err)
    _null_args(monkeypatch, "lk_ingest_batch", 11)
    got = _capi.ingest_batch(batch.time, batch.flux, batch.n_off, flux_err=batch.flux_err)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ref[:4], got[:4]))


def test_transit_mask_batch_and_single(golden):
    g = golden("ingest")
    batch, n = _batch(g)
    per = np.concatenate([g["period_%d" % b] for b in range(n)])
    dur = np.concatenate([g["duration_%d" % b] for b in range(n)])
    tt = np.concatenate([g["transit_time_%d" % b] for b in range(n)])
    poff = np.arange(n + 1) * 2
    mask = batch.create_transit_mask(per, tt, dur, planet_off=poff)
    for b in range(n):
        s = slice(batch.n_off[b], batch.n_off[b + 1])
        assert np.array_equal(mask[s], g["mask_%d" % b])
        one = batch[b].create_transit_mask(g["period_%d" % b], g["transit_time_%d" % b], g["duration_%d" % b])
        assert np.array_equal(one, g["mask_%d" % b])
    # negative periods / phases follow numpy's `%` (oracle)
    t = np.linspace(-7, 9, 4001)
    lc = LightCurve(time=t, flux=np.ones_like(t))
    for p, d, t0 in ((1.7, 0.3, 0.2), (-2.1, 0.4, 5.0), (3.0, 0.0, 1.0)):
        assert np.array_equal(lc.create_transit_mask(p, t0, d), O.transit_mask(t, p, d, t0))


def test_bin_batch_vs_reference(golden):
    from lightkurve_amd import _capi
    g = golden("ingest")
    batch, n = _batch(g)
    for b in range(n):                      # per light curve: its own bin size, as in the golden
        lc = batch[b]
        out = lc.bin(time_bin_size=float(g["bin_size_%d" % b]))
        assert out.time.shape == g["bin_time_%d" % b].shape
        assert np.allclose(out.time, g["bin_time_%d" % b], rtol=0, atol=1e-9)
        assert np.allclose(out.flux, g["bin_flux_%d" % b], rtol=1e-13, atol=0, equal_nan=True)
        assert np.allclose(out.flux_err, g["bin_err_%d" % b], rtol=1e-12, atol=0, equal_nan=True)
    # the whole ragged batch with one shared bin size in one launch == the oracle per light curve
    binned = batch.bin(time_bin_size=0.4)
    for b in range(n):
        rt, rf, re_ = O.bin_lightcurve(g["time_%d" % b], g["flux_%d" % b], g["err_%d" % b], 0.4)
        assert np.allclose(binned[b].time, rt, rtol=0, atol=1e-9)
        assert np.allclose(binned[b].flux, rf, rtol=1e-13, atol=0, equal_nan=True)
        assert np.allclose(binned[b].flux_err, re_, rtol=1e-12, atol=0, equal_nan=True)
    # no flux_err (NULL) bins like errors that are all NaN
    nan_err = np.full(batch.time.size, np.nan)
    ref = _capi.bin_batch(batch.time, batch.flux, batch.n_off, flux_err=nan_err, time_bin_size=0.4)
    got = _capi.bin_batch(batch.time, batch.flux, batch.n_off, time_bin_size=0.4)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ref, got))


def test_batch_feeds_the_periodogram_path():
    """ingest -> Lomb-Scargle without leaving the batch layout: same spectra as the per-light-curve route."""
    from lightkurve_amd import synth
    from lightkurve_amd.batch import lombscargle_batch
    lcs = []
    for i in range(5):
        t, y, e, _ = synth.ls_target(15, i, 1200 + 100 * i, cadence_days=10.0 / 1440.0)
        y = y.copy()
        y[[3, 500 + i]] = np.nan
        lcs.append(LightCurve(time=t + 100.0, flux=y * (2 + i), flux_err=e))
    batch = LightCurveBatch.from_lightcurves(lcs).normalize()
    f = 0.05 + 0.01 * np.arange(3000)
    P = batch.to_periodogram_power(f)
    ref = lombscargle_batch([lc.remove_nans().normalize() for lc in lcs], f)
    assert np.max(np.abs(P - ref)) <= 1e-12 * np.max(ref)


def test_fits_files_to_batch_vs_reference_readers(golden, monkeypatch):
    """FITS -> ragged arrays on the device (lk_fits_unpack_batch) for a mixed batch of Kepler-, TESS- and generic-layout
    files against what lightkurve's own readers return for the same files (oracle/gen_golden.py::gen_fits)."""
    import os
    from lightkurve_amd.ingest import LightCurveBatch
    g = golden("fits_ingest")
    fdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fits")
    paths = [os.path.join(fdir, n) for n in ("kepler_llc.fits", "tess_lc.fits", "generic_double.fits", "kepler_llc.fits")]
    batch = LightCurveBatch.from_fits(paths)
    tags = ["kepler_default", "tess_default", "generic", "kepler_default"]
    assert len(batch) == 4 and batch.n_off[-1] == sum(len(g[t + "_time"]) for t in tags)
    for b, tag in enumerate(tags):
        lc = batch[b]
        assert np.array_equal(lc.time, g[tag + "_time"]), tag
        assert np.array_equal(lc.flux, g[tag + "_flux"], equal_nan=True), tag
        assert np.array_equal(lc.flux_err, g[tag + "_flux_err"], equal_nan=True), tag
        if tag + "_quality" in g:
            assert np.array_equal(batch.quality[batch.n_off[b]:batch.n_off[b + 1]], g[tag + "_quality"]), tag
    assert batch.meta[0]["MISSION"] == "Kepler" and batch.meta[1]["LABEL"] == "SYNTH tess_lc"
    # reader options: SAP flux + 'hard' mask, no mask, an integer mask
    for kw, tag, path in [(dict(flux_column="sap_flux", quality_bitmask="hard"), "kepler_hard_sap", paths[0]),
                          (dict(quality_bitmask="none"), "kepler_none", paths[0]),
                          (dict(quality_bitmask=2 + 8 + 128), "tess_int", paths[1])]:
        one = LightCurveBatch.from_fits([path], **kw)
        assert np.array_equal(one.time, g[tag + "_time"]) and np.array_equal(one.flux, g[tag + "_flux"], equal_nan=True)
        assert np.array_equal(one.flux_err, g[tag + "_flux_err"], equal_nan=True)
        assert np.array_equal(one.quality, g[tag + "_quality"])
    # the batch goes straight on: remove_nans + normalize + periodogram of the Kepler file
    raw2 = LightCurveBatch.from_fits(paths[:2])
    clean = raw2.remove_nans().normalize()
    assert np.isfinite(clean.flux).all() and abs(np.median(clean[0].flux) - 1.0) < 1e-12
    # the quality flags stay in step with the cadences that survive (reference: lc.remove_nans() keeps lc.quality aligned)
    assert clean.quality is not None and len(clean.quality) == len(clean.time)
    assert np.array_equal(clean.quality, raw2.quality[~np.isnan(raw2.flux)])
    assert clean.bin(time_bin_size=0.5).quality is None
    # many files: more workgroups than one wave of CUs, records staged through LDS in several trips
    big = LightCurveBatch.from_fits(paths[:3] * 40)
    assert len(big) == 120 and np.array_equal(big[117].time, g["kepler_default_time"])
    # flux_err_out and quality_out NULL: the same cadences and flux
    _null_args(monkeypatch, "lk_fits_unpack_batch", 8, 9)
    bare = LightCurveBatch.from_fits(paths)
    assert np.array_equal(bare.n_off, batch.n_off) and np.array_equal(bare.time, batch.time)
    assert np.array_equal(bare.flux, batch.flux, equal_nan=True)


def test_read_dispatches_on_file_type(golden, monkeypatch):
    """lightkurve_amd.read(path): light-curve files -> LightCurve, target-pixel files -> PixelCube (reference io/read.py)."""
    import os
    import lightkurve_amd as lka
    from lightkurve_amd.correctors.pldcorrector import PixelCube
    g = golden("fits_ingest")
    fdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fits")
    lc = lka.read(os.path.join(fdir, "tess_lc.fits"))
    assert isinstance(lc, LightCurve) and np.array_equal(lc.time, g["tess_default_time"])
    assert np.array_equal(lc.flux, g["tess_default_flux"], equal_nan=True) and lc.meta["MISSION"] == "TESS"
    hard = lka.read(os.path.join(fdir, "kepler_llc.fits"), quality_bitmask="hard", flux_column="sap_flux")
    assert np.array_equal(hard.flux, g["kepler_hard_sap_flux"], equal_nan=True)
    cube = lka.read(os.path.join(fdir, "kepler_tpf.fits"))
    assert isinstance(cube, PixelCube) and np.array_equal(cube.flux, g["ktpf_default_flux"], equal_nan=True)
    # lk_fits_unpack_cube with quality_out NULL: the same times and cubes
    _null_args(monkeypatch, "lk_fits_unpack_cube", 14)
    bare = lka.read(os.path.join(fdir, "kepler_tpf.fits"))
    assert np.array_equal(bare.time, cube.time, equal_nan=True) and np.array_equal(bare.flux, cube.flux, equal_nan=True)
    assert np.array_equal(bare.flux_err, cube.flux_err, equal_nan=True)


def test_median_of_long_light_curves_is_the_exact_order_statistic():
    """The sampled select behind `normalize` (block_select.hpp) on inputs whose bracket overflows its LDS list (> ~50 000
    values): the histogram refinement must return numpy's nanmedian exactly — odd and even counts (the two middle ranks may
    fall into different bins), smooth and clustered values, heavy ties inside the bracket (the refinement gives up: radix
    select), a constant series, and NaNs that change the count."""
    from lightkurve_amd import _capi
    rng = np.random.default_rng(12)
    cases = {
        "gauss_odd": rng.standard_normal(200_001),
        "gauss_even": rng.standard_normal(300_000),
        "lognormal": np.exp(3 * rng.standard_normal(150_000)),
        "two_clusters": np.concatenate([rng.normal(0, 1e-6, 90_000), rng.normal(5, 1e-6, 90_000)]),  # the middle ranks straddle the gap
        "heavy_ties": np.round(rng.standard_normal(180_000), 2),
        "constant": np.full(120_000, 3.25),
        "with_nans": np.where(rng.random(250_000) < 0.1, np.nan, rng.standard_normal(250_000) ** 3),
        "tiny_spread": 1.0 + 1e-15 * rng.integers(0, 50, 140_000),
    }
    for name, f in cases.items():
        t = np.arange(f.size, dtype=np.float64)
        _, _, _, _, med = _capi.ingest_batch(t, f, np.array([0, f.size]), normalize=False)
        assert med[0] == np.nanmedian(f), name
    # several long light curves of different lengths in one call
    fs = [rng.standard_normal(n) for n in (70_000, 130_001, 55_000)]
    off = np.concatenate([[0], np.cumsum([f.size for f in fs])])
    _, _, _, _, med = _capi.ingest_batch(np.arange(off[-1], dtype=np.float64), np.concatenate(fs), off, normalize=False)
    assert np.array_equal(med, [np.median(f) for f in fs])


def test_median_over_value_families_sizes_and_orders_is_the_exact_order_statistic():
    """`normalize`'s instantiation of the sampled select (its lambdas, its out-of-line radix fallback, its LDS plan) on the
    inputs tests/test_block_select_gpu.py feeds the header directly: every value family (ties, both zeros, +-inf, denormals, a
    spread whose hi - lo overflows, ...) at every size up to 30 000, shuffled, ascending and descending, and the order that
    defeats the strided sample — one ragged call.  The median is an order statistic or the IEEE mean of two: `==` (value
    equality, NaN where the reference is NaN: the mean of -inf and +inf), and normalised flux == flux / median bit for bit."""
    from lightkurve_amd import _capi
    from tests import select_harness as SH
    cases = SH.production_batch()
    flux = np.concatenate([v for _, v in cases])
    off = np.concatenate([[0], np.cumsum([v.size for _, v in cases])])
    t = np.arange(flux.size, dtype=np.float64)
    ref = np.array([SH.reference_median(v) for _, v in cases])
    to, fo, _, new_off, med = _capi.ingest_batch(t, flux, off, normalize=False)
    assert np.array_equal(new_off, off) and np.array_equal(fo, flux) and np.array_equal(to, t)   # nothing to drop: no NaN flux
    bad = [cases[b][0] for b in np.flatnonzero(~((med == ref) | (np.isnan(med) & np.isnan(ref))))]
    assert not bad, bad
    _, fn, _, _, med2 = _capi.ingest_batch(t, flux, off, normalize=True)
    assert np.array_equal(med2, med, equal_nan=True)
    with np.errstate(all="ignore"):
        want = flux / np.repeat(med, np.diff(off))        # (by the median the device returned: a zero median keeps ITS sign)
    bad = [cases[b][0] for b in range(len(cases))
           if not np.array_equal(fn[off[b]:off[b + 1]], want[off[b]:off[b + 1]], equal_nan=True)]
    assert not bad, bad
