"""GPU: DevicePixelCubeBatch — target-pixel cutouts resident in HBM, PLD without host gathers.  The contract is EQUALITY OF
BITS with ``pld_correct_batch`` on the same cutouts (the same PLD kernels must be handed the same numbers by the new
preparation kernels), plus the reference's own golden at the benchmark shape."""
import hashlib
import os

import numpy as np
import pytest

from lightkurve_amd import _capi, synth
from lightkurve_amd.correctors import PixelCube, pld_correct_batch
from lightkurve_amd.correctors.pldcorrector import _batch_cutout, _percentile_knots
from lightkurve_amd.device import DeviceLightCurveBatch, DevicePixelCubeBatch
from tests.test_pixcube_cpu import aperture_cases

pytestmark = pytest.mark.gpu

FITS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fits")


def cubes_equal(a, b):
    return (np.array_equal(a.time, b.time, equal_nan=True) and a.flux.dtype == b.flux.dtype == np.float32
            and np.array_equal(a.flux, b.flux, equal_nan=True) and np.array_equal(a.flux_err, b.flux_err, equal_nan=True))


def front_end_cubes(n=800, npix=9, seeds=(50, 51, 52)):
    """The cutouts of test_batch_front_end_matches_the_per_object_corrector: 4 all-NaN and 3 all-zero cadences per cutout, at
    different places."""
    rng = np.random.default_rng(8)
    cubes = []
    for s in seeds:
        t, flux, err, _ = synth.pld_cutout(4, s, n=n, npix=npix)
        flux, err = flux.copy(), err.copy()
        bad = rng.choice(n, 7, replace=False)
        flux[bad[:4]] = np.nan
        flux[bad[4:]] = 0.0
        cubes.append(PixelCube(t, flux, err, mission="K2"))
    return cubes


def front_end_masks():
    ap = np.zeros((9, 9), bool)
    ap[2:7, 2:7] = True
    pm = np.zeros((9, 9), bool)
    pm[1:8, 1:8] = True
    return ap, pm, ~ap


# ------------------------------------------------------------------------------------------------ 1. round trips
def test_round_trip_from_cubes_and_arrays():
    cubes = front_end_cubes()
    back = DevicePixelCubeBatch.from_cubes(cubes).to_host()
    assert len(back) == 3 and all(cubes_equal(a, b) for a, b in zip(cubes, back))
    assert back[1].meta["MISSION"] == "K2"
    t = np.stack([c.time for c in cubes])
    f, e = np.stack([c.flux for c in cubes]), np.stack([c.flux_err for c in cubes])
    batch = DevicePixelCubeBatch.from_arrays(t, f, e)
    assert batch.shape == (3, 800, 9, 9) and len(batch) == 3
    assert all(cubes_equal(a, b) for a, b in zip(cubes, batch.to_host()))


@pytest.mark.parametrize("fname", ["kepler_tpf.fits", "tess_tpf.fits"])
@pytest.mark.parametrize("bitmask", ["default", "none"])
def test_round_trip_from_fits(fname, bitmask):
    path = os.path.join(FITS, fname)
    ref = PixelCube.from_fits(path, quality_bitmask=bitmask)
    batch = DevicePixelCubeBatch.from_fits([path, path], quality_bitmask=bitmask)
    assert batch.shape == (2,) + ref.shape
    back = batch.to_host()
    assert cubes_equal(back[0], ref) and cubes_equal(back[1], ref)
    assert back[0].meta["MISSION"] == ref.meta["MISSION"] and back[1].meta["TARGETID"] == ref.meta["TARGETID"]


def test_from_fits_needs_one_cadence_count():
    path = os.path.join(FITS, "tess_tpf.fits")
    with pytest.raises(ValueError):
        DevicePixelCubeBatch.from_fits([os.path.join(FITS, "kepler_tpf.fits"), path], quality_bitmask="default")


# ------------------------------------------------------------------------------------------------ 2. aperture photometry
@pytest.mark.parametrize("npix", [9, 10, 11])
def test_to_lightcurves_equals_numpy_aperture_sums(npix):
    """9 x 9: odd LDS pitch; 10 x 10: even, padded by one dword; 11 x 11: the benchmark's."""
    for name, cube, ap in aperture_cases(npix):
        lc = cube.to_lightcurve(ap)
        flux, err = np.asarray(lc.flux, dtype=np.float64), np.asarray(lc.flux_err, dtype=np.float64)
        keep = ~(np.isnan(flux) | np.isnan(err))
        assert 600 < keep.sum() <= 700
        got = DevicePixelCubeBatch.from_cubes([cube, cube]).to_lightcurves(ap).to_host()
        n = int(keep.sum())
        assert np.array_equal(got.n_off, [0, n, 2 * n]), name
        for b in range(2):
            sl = slice(b * n, (b + 1) * n)
            assert np.array_equal(got.time[sl], cube.time[keep]), name
            assert np.array_equal(got.flux[sl], flux[keep]), name
            assert np.array_equal(got.flux_err[sl], err[keep]), name


def test_to_lightcurves_wide_cutout_is_walked_in_chunks():
    """More pixels than one LDS chunk holds (15 x 15 = 225 > 127): the running float32 sums carry over the chunks."""
    t, flux, err, _ = synth.pld_cutout(4, 9, n=200, npix=15)
    flux = flux.copy()
    flux[7] = np.nan
    flux[9, 3, 4] = np.nan
    ap = np.ones((15, 15), bool)
    ap[:, :2] = False
    cube = PixelCube(t, flux, err)
    ref_f, ref_e = cube._aperture_sums(ap)
    keep = ~(np.isnan(ref_f) | np.isnan(ref_e))
    got = DevicePixelCubeBatch.from_cubes([cube]).to_lightcurves(ap).to_host()
    assert np.array_equal(got.flux, ref_f[keep].astype(np.float64)) and np.array_equal(got.flux_err, ref_e[keep].astype(np.float64))


# ------------------------------------------------------------------------------------------------ 3. the contract
def test_pld_correct_equals_host_path_and_reference_golden(golden):
    """(a) golden pld_c5: 11 x 11 x 3500, order 3, 16 components, all pixels — the zero-copy route (the PLD block IS the
    resident cube)."""
    g = golden("pld_c5")
    cubes = []
    for i in range(int(g["n_cutouts"])):
        t, flux, err, _ = synth.pld_cutout(4, i, n=3500, npix=11)
        assert hashlib.sha256(t.tobytes() + flux.tobytes() + err.tobytes()).hexdigest() == str(g["sha_%d" % i])
        cubes.append(PixelCube(g["time_%d" % i], flux, err, mission="K2"))
    corrected, outl = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(pld_order=3, pca_components=16)
    ref_c, ref_o = pld_correct_batch(cubes, pld_order=3, pca_components=16)
    assert corrected.shape == ref_c.shape and outl.dtype == bool
    assert np.array_equal(corrected, ref_c) and np.array_equal(outl, ref_o)
    for i in range(len(cubes)):
        assert np.array_equal(outl[i], g["outlier_mask_%d" % i]), i
        assert np.max(np.abs(corrected[i] - g["corrected_%d" % i])) / np.median(g["corrected_%d" % i]) < 1e-6, i


@pytest.mark.parametrize("restore", [True, False])
def test_pld_correct_partial_masks_and_dropped_cadences(restore):
    """(b) partial SAP aperture, distinct PLD / background masks, 4 all-NaN and 3 all-zero cadences per cutout."""
    cubes = front_end_cubes()
    ap, pm, bm = front_end_masks()
    kw = dict(aperture_mask=ap, pld_aperture_mask=pm, background_aperture_mask=bm, pld_order=2, pca_components=8,
              restore_trend=restore)
    corrected, outl = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(**kw)
    ref_c, ref_o = pld_correct_batch(cubes, **kw)
    assert corrected.shape == (3, 793)
    assert np.array_equal(corrected, ref_c) and np.array_equal(outl, ref_o)
    # all pixels with dropped cadences (one gathered block for both operands), and equal partial masks
    for kw in (dict(pld_order=2, pca_components=8), dict(pld_aperture_mask=pm, background_aperture_mask=pm, pld_order=1, pca_components=6)):
        corrected, outl = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(aperture_mask=ap, restore_trend=restore, **kw)
        ref_c, ref_o = pld_correct_batch(cubes, aperture_mask=ap, restore_trend=restore, **kw)
        assert np.array_equal(corrected, ref_c) and np.array_equal(outl, ref_o)


def test_pld_correct_with_cadence_mask():
    """(c) a cadence mask with a hole, against lk_pld_correct_batch fed by _batch_cutout's arrays."""
    cubes = front_end_cubes()
    ap, pm, bm = front_end_masks()
    parts = [_batch_cutout(c, ap, pm, bm, (ap, pm, bm)) for c in cubes]
    n = len(parts[0][0])
    t, y, err = (np.stack([p[k] for p in parts]) for k in (0, 1, 2))
    lcf, pld, bkg = (np.ascontiguousarray(np.stack([p[k] for p in parts])) for k in (3, 4, 5))
    knots = np.stack([_percentile_knots(t[b], n // 50, 5) for b in range(3)])
    cm = np.ones((3, n), bool)
    cm[1, 100:140] = False
    cm[2, 700:] = False
    res = _capi.pld_correct_batch(pld, bkg, lcf, t, knots, y, err, 2, 8, 5, True, cadence_mask=cm, sigma=5, niters=5)
    ref = y - res["model"]
    ref += res["spline"] - np.median(res["spline"], axis=1)[:, None]
    corrected, outl = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(
        aperture_mask=ap, pld_aperture_mask=pm, background_aperture_mask=bm, pld_order=2, pca_components=8, cadence_mask=cm)
    assert np.array_equal(corrected, ref) and np.array_equal(outl, res["outlier_mask"])
    with pytest.raises(ValueError, match="cadence_mask"):
        DevicePixelCubeBatch.from_cubes(cubes).pld_correct(aperture_mask=ap, cadence_mask=np.ones((3, 800), bool))


def test_pld_correct_without_pixel_block():
    """(d) pld_aperture_mask='empty': background + spline only."""
    cubes = [PixelCube(*synth.pld_cutout(4, 60 + i, n=900, npix=7)[:3], mission="K2") for i in range(2)]
    kw = dict(pld_aperture_mask="empty", pld_order=1, pca_components=3)
    corrected, outl = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(**kw)
    ref_c, ref_o = pld_correct_batch(cubes, **kw)
    assert np.array_equal(corrected, ref_c) and np.array_equal(outl, ref_o)


# ------------------------------------------------------------------------------------------------ 4. data-dependent masks
def rolled_cubes(widen_last=False):
    """Three copies of ONE cutout rolled by (-1, 0, +1) pixels, the same two NaN and two zero cadences in each;
    ``widen_last``: the last copy's star is doubled sideways, so its threshold mask has another size."""
    t, flux, err, _ = synth.pld_cutout(4, 70, n=700, npix=9)
    cubes = []
    for sh in (-1, 0, 1):
        f = np.roll(flux, (sh, -sh), axis=(1, 2))
        if widen_last and sh == 1:
            f = (f + np.roll(f, 2, axis=2) - np.float32(50.0)).astype(np.float32)
        f[[30, 400]] = np.nan
        f[[31, 500]] = 0.0
        cubes.append(PixelCube(t, f, np.roll(err, (sh, -sh), axis=(1, 2)), mission="K2"))
    return cubes


def test_data_dependent_masks_are_resolved_per_cutout():
    cubes = rolled_cubes()
    masks = [c.create_threshold_mask(3) for c in cubes]
    assert all(m.sum() == 25 for m in masks) and not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    med = batch.median_images()
    with np.errstate(all="ignore"):
        for b, c in enumerate(cubes):
            assert np.array_equal(med[b], np.nanmedian(c.flux.astype(np.float64), axis=0)), b
    kw = dict(aperture_mask=None, pld_aperture_mask="threshold", background_aperture_mask="background", pld_order=2,
              pca_components=8)
    corrected, outl = batch.pld_correct(**kw)
    ref_c, ref_o = pld_correct_batch(cubes, **kw)
    assert corrected.shape == (3, 696)
    assert np.array_equal(corrected, ref_c) and np.array_equal(outl, ref_o)
    # per-cutout photometric aperture alone (shared PLD / background masks)
    corrected, outl = batch.pld_correct(aperture_mask=None, pld_order=2, pca_components=8)
    ref_c, ref_o = pld_correct_batch(cubes, aperture_mask=None, pld_order=2, pca_components=8)
    assert np.array_equal(corrected, ref_c) and np.array_equal(outl, ref_o)


def test_median_image_with_nan_pixels_and_kept_cadences_only():
    t, flux, err, _ = synth.pld_cutout(4, 73, n=333, npix=6)             # even and odd counts per pixel, 36 pixels: 3 groups
    flux = flux.copy()
    rng = np.random.default_rng(3)
    flux[rng.integers(333, size=200), rng.integers(6, size=200), rng.integers(6, size=200)] = np.nan
    flux[[4, 5]] = 0.0
    flux[:, 5, 5] = np.nan                                                 # a pixel without any value (set last: no zeros in it)
    cube = PixelCube(t, flux, err)
    batch = DevicePixelCubeBatch.from_cubes([cube, cube])
    with np.errstate(all="ignore"):
        ref = np.nanmedian(flux.astype(np.float64), axis=0)
    med = batch.median_images()
    assert np.isnan(ref[5, 5]) and np.isfinite(np.delete(ref.ravel(), 35)).all()
    assert np.array_equal(med[0], ref, equal_nan=True) and np.array_equal(med[1], ref, equal_nan=True) and np.isnan(med[0, 5, 5])


def test_data_dependent_masks_of_different_sizes_are_refused():
    cubes = rolled_cubes(widen_last=True)
    kw = dict(aperture_mask="all", pld_aperture_mask="threshold", background_aperture_mask="background", pld_order=2,
              pca_components=8)
    with pytest.raises(ValueError, match="different numbers of pixels"):
        pld_correct_batch(cubes, **kw)
    with pytest.raises(ValueError, match="different numbers of pixels"):
        DevicePixelCubeBatch.from_cubes(cubes).pld_correct(**kw)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_bad_input_is_a_value_error():
    cubes = front_end_cubes()
    ap, pm, bm = front_end_masks()
    with pytest.raises(ValueError, match="one shape"):                                       # mixed shapes
        DevicePixelCubeBatch.from_cubes(cubes + [PixelCube(cubes[0].time[:-1], cubes[0].flux[:-1], cubes[0].flux_err[:-1])])
    f = cubes[1].flux.copy()                                                                 # different kept counts
    f[np.flatnonzero(np.isfinite(f[:, 4, 4]) & (f[:, 4, 4] != 0))[0]] = np.nan
    uneven = [cubes[0], PixelCube(cubes[1].time, f, cubes[1].flux_err), cubes[2]]
    with pytest.raises(ValueError, match="same number of valid cadences"):
        DevicePixelCubeBatch.from_cubes(uneven).pld_correct(aperture_mask=ap, pld_order=2, pca_components=8)
    with pytest.raises(ValueError, match="same number of valid cadences"):
        DevicePixelCubeBatch.from_cubes(uneven).to_lightcurves(ap)
    # a non-finite pixel inside the PLD mask of a kept cadence (outside the photometric aperture, so the cadence is kept)
    for val in (np.nan, np.inf):
        f = cubes[0].flux.copy()
        row = np.flatnonzero(np.isfinite(f[:, 4, 4]) & (f[:, 4, 4] != 0))[5]
        f[row, 1, 1] = val
        dirty = [PixelCube(cubes[0].time, f, cubes[0].flux_err), cubes[1], cubes[2]]
        for kw in (dict(pld_aperture_mask=pm, background_aperture_mask=bm), dict()):        # gathered blocks; all pixels
            with pytest.raises(ValueError, match="finite pixels inside the masks"):
                DevicePixelCubeBatch.from_cubes(dirty).pld_correct(aperture_mask=ap, pld_order=2, pca_components=8, **kw)
    # ... and with no dropped cadence, where the block is the resident cube itself
    clean = [PixelCube(*synth.pld_cutout(4, 80 + i, n=300, npix=9)[:3]) for i in range(2)]
    f = clean[1].flux.copy()
    f[17, 0, 8] = np.nan
    with pytest.raises(ValueError, match="finite pixels inside the masks"):
        DevicePixelCubeBatch.from_cubes([clean[0], PixelCube(clean[1].time, f, clean[1].flux_err)]).pld_correct(
            aperture_mask=ap, pld_order=1, pca_components=4)
    # unsorted times
    t = clean[0].time.copy()
    t[[10, 11]] = t[[11, 10]]
    with pytest.raises(ValueError, match="non-decreasing"):
        DevicePixelCubeBatch.from_cubes([PixelCube(t, clean[0].flux, clean[0].flux_err), clean[1]]).pld_correct(
            pld_order=1, pca_components=4)
    # a knot count the spline degree cannot carry
    with pytest.raises(ValueError, match="too small"):
        DevicePixelCubeBatch.from_cubes(clean).pld_correct(pld_order=1, pca_components=4, spline_n_knots=3)


# ------------------------------------------------------------------------------------------------ 6. chaining
def test_resident_result_chains_into_flatten():
    cubes = front_end_cubes()
    ap, pm, bm = front_end_masks()
    kw = dict(aperture_mask=ap, pld_aperture_mask=pm, background_aperture_mask=bm, pld_order=2, pca_components=8)
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    corrected, outl = batch.pld_correct(**kw)
    dev, d_outl = batch.pld_correct(to_host=False, **kw)
    assert isinstance(dev, DeviceLightCurveBatch)
    host = dev.to_host()
    B, n = corrected.shape
    assert np.array_equal(host.n_off, np.arange(B + 1) * n)
    assert np.array_equal(host.flux.reshape(B, n), corrected)
    assert np.array_equal(d_outl.download(np.uint8, B * n).reshape(B, n).astype(bool), outl)
    for b, c in enumerate(cubes):
        f32, e32 = c._aperture_sums(ap)
        keep = ~(np.isnan(f32) | np.isnan(e32))
        assert np.array_equal(host.time.reshape(B, n)[b], c.time[keep])
        assert np.array_equal(host.flux_err.reshape(B, n)[b], e32[keep].astype(np.float64))
    flat = dev.flatten(window_length=101).to_host()
    ref = DeviceLightCurveBatch.from_arrays(host.time, host.flux, host.flux_err, host.n_off).flatten(window_length=101).to_host()
    assert np.array_equal(flat.flux, ref.flux, equal_nan=True) and np.array_equal(flat.flux_err, ref.flux_err, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_run_twice_same_bits():
    cubes = front_end_cubes()
    ap, pm, bm = front_end_masks()
    kw = dict(aperture_mask=ap, pld_aperture_mask=pm, background_aperture_mask=bm, pld_order=2, pca_components=8)
    batch = DevicePixelCubeBatch.from_cubes(cubes)
    a = batch.pld_correct(**kw)
    b = batch.pld_correct(**kw)
    t, y, e, off = synth.ls_batch(21, 3, 4000)                       # other work in between: different scratch contents
    _capi.ls_fast_batch(t - t[0], y, off, f0=0.01, df=0.01, M=20000, normalization="psd")
    c = DevicePixelCubeBatch.from_cubes(cubes).pld_correct(**kw)
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])
    la, lb = batch.to_lightcurves(None).to_host(), batch.to_lightcurves(None).to_host()
    assert np.array_equal(la.flux, lb.flux) and np.array_equal(la.flux_err, lb.flux_err)
