"""CPU: the host half of DevicePixelCubeBatch.  The resident PLD path must hand the PLD kernels exactly the numbers
``pld_correct_batch`` does, so the three facts the device kernels rely on are pinned here against numpy itself:
the summation order of ``PixelCube._aperture_sums``, the index / weight plan behind ``np.percentile`` and the split of
``create_threshold_mask`` into "median image" + "mask from median image"."""
import ctypes

import numpy as np
import pytest

from lightkurve_amd import _capi, synth
from lightkurve_amd.correctors.pldcorrector import (PixelCube, _knots_from_plan, _percentile_knot_plan, _percentile_knots,
                                                    _sequential_aperture_sums, threshold_mask_from_median_image)

NEW_SYMBOLS = ("lk_cube_aperture_batch_dev", "lk_cube_median_image_batch_dev", "lk_pld_gather_batch_dev",
               "lk_pld_correct_batch_dev")


def aperture_cases(npix=11, n=700, seed=4):
    """(name, PixelCube, aperture) — full and partial aperture, all-finite and with NaN pixels, an all-NaN cadence, an
    all-zero cadence, NaN errors."""
    t, flux, err, _ = synth.pld_cutout(4, seed, n=n, npix=npix)
    rng = np.random.default_rng(seed)
    full = np.ones((npix, npix), bool)
    part = np.zeros((npix, npix), bool)
    part[2:npix - 2, 3:npix - 1] = True
    part[0, 0] = True
    dirty_f, dirty_e = flux.copy(), err.copy()
    for _ in range(60):                                   # scattered NaN pixels, inside and outside the partial aperture
        dirty_f[rng.integers(n), rng.integers(npix), rng.integers(npix)] = np.nan
    dirty_f[17] = np.nan                                  # all-NaN cadence
    dirty_f[40] = 0.0                                     # all-zero cadence
    dirty_f[41][part] = 0.0                               # zero inside the aperture only: flux 0, not NaN
    dirty_f[55][part] = np.nan                            # no finite pixel inside the aperture
    dirty_e[23, 4, 5] = np.nan                            # NaN errors
    dirty_e[300] = np.nan
    zero_f = flux.copy()
    zero_f[100] = 0.0                                     # all finite, one all-zero cadence (the fast branch's own rule)
    out = []
    for cname, f, e in (("finite", flux, err), ("zero_cadence", zero_f, err), ("nan", dirty_f, dirty_e)):
        for aname, ap in (("full", full), ("partial", part)):
            out.append(("%s-%s-%d" % (cname, aname, npix), PixelCube(t, f, e, mission="K2"), ap))
    return out


@pytest.mark.parametrize("npix", [9, 10, 11])
def test_sequential_float32_sums_equal_numpy_aperture_sums(npix):
    for name, cube, ap in aperture_cases(npix):
        ref_f, ref_e = cube._aperture_sums(ap)
        got_f, got_e = _sequential_aperture_sums(cube.flux, cube.flux_err, ap)
        assert ref_f.dtype == np.float32 and ref_e.dtype == np.float32, name
        assert np.array_equal(got_f, ref_f, equal_nan=True), name
        assert np.array_equal(got_e, ref_e, equal_nan=True), name
        if name.startswith("nan"):
            assert np.isnan(ref_f[17]) and np.isnan(ref_f[40]) and np.isnan(ref_f).sum() < 10, name
            assert np.isfinite(ref_e).all(), name


@pytest.mark.parametrize("n,n_knots,degree", [(3467, 69, 5), (3500, 70, 5), (793, 15, 5), (696, 13, 3), (500, 6, 5), (50, 4, 3),
                                               (1001, 20, 5), (2, 6, 5), (700, 14, 1)])
def test_knot_plan_and_lerp_equal_np_percentile(n, n_knots, degree):
    rng = np.random.default_rng(n)
    t = np.cumsum(rng.uniform(0.0, 0.05, n)) + 2454833.0 * rng.integers(0, 2)       # non-decreasing, uneven, large offsets too
    t[n // 2:] += 3.7                                                                # a gap
    lo, g = _percentile_knot_plan(n, n_knots, degree)
    assert lo.dtype == np.int32 and g.dtype == np.float64 and len(lo) == len(g) == n_knots - degree - 1
    assert np.all((lo >= 0) & (lo < n)) and np.all((g >= 0) & (g < 1))
    assert np.array_equal(_knots_from_plan(t, lo, g), _percentile_knots(t, n_knots, degree))


def test_knot_plan_rejects_too_few_knots():
    with pytest.raises(ValueError, match="too small"):
        _percentile_knot_plan(100, 3, 5)


def test_mask_from_median_image_equals_create_threshold_mask():
    for seed, npix in ((70, 9), (71, 11), (72, 10)):
        t, flux, err, _ = synth.pld_cutout(4, seed, n=700, npix=npix)
        flux = flux.copy()
        flux[[5, 300]] = np.nan
        flux[[6, 301]] = 0.0
        flux[10, 1, 2] = np.nan
        cube = PixelCube(t, flux, err, mission="K2")
        with np.errstate(all="ignore"):
            med = np.nanmedian(flux.astype(np.float64), axis=0)
        for kw in (dict(threshold=3, reference_pixel="center"), dict(threshold=0, reference_pixel=None), dict(threshold=3)):
            m = threshold_mask_from_median_image(med, **kw)
            assert m.dtype == bool and m.shape == (npix, npix)
            assert np.array_equal(m, cube.create_threshold_mask(**kw)), (seed, kw)
        assert 0 < threshold_mask_from_median_image(med, 3).sum() < npix * npix
    # an all-NaN pixel stays outside the mask, as in the method
    flux[:, 0, 0] = np.nan
    with np.errstate(all="ignore"):
        med = np.nanmedian(flux.astype(np.float64), axis=0)
    assert np.array_equal(threshold_mask_from_median_image(med, 0, None), PixelCube(t, flux, err).create_threshold_mask(0, None))


def test_new_entry_points_are_bound_and_exported():
    names = [s[0] for s in _capi.SIGNATURES]
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert names.count(sym) == 1, sym
        assert hasattr(lib, sym), sym
    from lightkurve_amd import device
    assert "DevicePixelCubeBatch" in device.__all__


def test_device_batch_is_float32_only():
    """The device batch holds float32 cubes; anything else is a TypeError before the device is touched."""
    from lightkurve_amd.device import DevicePixelCubeBatch
    t, flux, err, _ = synth.pld_cutout(4, 1, n=60, npix=5)
    with pytest.raises(TypeError, match="float32"):
        DevicePixelCubeBatch.from_cubes([PixelCube(t, flux.astype(np.float64), err.astype(np.float64))])
    with pytest.raises(TypeError, match="float32"):
        DevicePixelCubeBatch.from_arrays(t[None], flux[None].astype(np.float64), err[None])
    with pytest.raises(ValueError, match="one shape"):
        DevicePixelCubeBatch.from_cubes([PixelCube(t, flux, err), PixelCube(t[:-1], flux[:-1], err[:-1])])
