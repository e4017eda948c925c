"""GPU: the resident amplitude images (csrc/ampimage.hip: cube_ampimage_*_kernel, ampimage_offsets_kernel) against the numpy
mirror PixelCube.amplitude_image on the cases of tests/ampimage_cases.py.

Bounds: counts, statuses and NaN patterns exact; theta, level, amplitude, amplitude_err and chi2 1e-9 of the image's largest
finite |value| (the house rule: float64 sums of at most 300 float32 values in another order and another elimination order of a
well-conditioned K x K system, ~1e-13); phase 1e-9 rad where the amplitude exceeds 1e-3 of its maximum (below that the phase is
ill-defined by construction, and theta is compared there); centroids and offsets 1e-9 px.  Every comparison prints its largest
difference before it asserts."""
import functools

import numpy as np
import pytest

import ampimage_cases as C
from lightkurve_amd import batch
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.device import DeviceBuffer, DevicePixelCubeBatch

pytestmark = pytest.mark.gpu

SCALED = ("theta", "level", "amplitude", "amplitude_err", "chi2")
FLOAT_IMAGES = SCALED + ("phase", "snr")
CENTROIDS = ("centroid_amp", "centroid_level", "centroid_amp_moments", "centroid_level_moments", "offset", "offset_pix")


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def max_diff(a, b):
    ok = np.isfinite(np.asarray(b, dtype=np.float64))
    return float(np.max(np.abs(np.asarray(a)[ok] - np.asarray(b)[ok]))) if ok.any() else 0.0


def cubes_of(shape, N, nterms):
    time, flux, err, f = C.case(shape, N, nterms)
    return DevicePixelCubeBatch.from_arrays(time, flux, err)


@functools.lru_cache(maxsize=None)
def device_result(shape, N, nterms):
    """amplitude_images of the three cutouts of C.case in one batch, each at its own frequency; shared, read-only."""
    return cubes_of(shape, N, nterms).amplitude_images(C.case(shape, N, nterms)[3], nterms)


def check_against(got, ref, what):
    for key in ("status", "n_used"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], ref[key]), (what, key)
    assert np.array_equal(got["t_ref"], ref["t_ref"], equal_nan=True) and np.array_equal(got["frequency"], ref["frequency"], equal_nan=True)
    for key in FLOAT_IMAGES:
        assert got[key].shape == ref[key].shape and same_nan(got[key], ref[key]), (what, key)
    for key in SCALED:
        for b in range(len(ref[key])):
            top = np.abs(ref[key][b][np.isfinite(ref[key][b])])
            if top.size == 0 or top.max() == 0:
                continue
            err = max_diff(got[key][b], ref[key][b]) / top.max()
            print("%s cutout %d %s: max |device - mirror| / max |image| = %.3g" % (what, b, key, err))
            assert err < 1e-9, (what, key, b)
    amp = ref["amplitude"]
    with np.errstate(invalid="ignore"):
        defined = amp > 1e-3 * np.nanmax(np.where(np.isfinite(amp), amp, -np.inf), axis=(-2, -1), keepdims=True)
    if defined.any():
        turn = np.abs((got["phase"][defined] - ref["phase"][defined] + np.pi) % (2 * np.pi) - np.pi)
        print("%s phase: max |device - mirror| = %.3g rad over %d of %d pixels" % (what, turn.max(), defined.sum(), amp.size))
        assert turn.max() < 1e-9, what
    for key in CENTROIDS:
        assert same_nan(got[key], ref[key]), (what, key)
        err = max_diff(got[key], ref[key])
        print("%s %s: max |device - mirror| = %.3g px" % (what, key, err))
        assert err < 1e-9, (what, key)


# ------------------------------------------------------------------------------------------------ device against the mirror
@pytest.mark.parametrize("nterms", [1, 2, 3])
@pytest.mark.parametrize("N", C.NS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_amplitude_images_against_the_mirror(shape, N, nterms):
    got, ref = device_result(shape, N, nterms), C.mirror(shape, N, nterms)
    K = 2 * nterms + 1
    assert got["theta"].shape == (C.B, K) + shape and got["amplitude"].shape == (C.B, nterms) + shape
    assert got["level"].shape == got["n_used"].shape == (C.B,) + shape and got["centroid_amp"].shape == (C.B, 2)
    check_against(got, ref, "%s N=%d nterms=%d" % (shape, N, nterms))
    time = C.case(shape, N, nterms)[0]
    fitted = np.isfinite(time).sum(axis=1) >= K + 1
    assert np.array_equal(got["status"] == 2, ~fitted)
    if fitted[0]:                                    # what the special pixels of cutout 0 are for
        n = got["n_used"][0]
        assert n[0, 0] == 0 and n[0, 1] == min(K, n[1, 1]) and n[0, 2] == K - 1
        assert np.isnan(got["level"][0, 0, 0]) and np.isnan(got["level"][0, 0, 2]) and not np.isnan(got["level"][0, 0, 1])
        assert np.isnan(got["amplitude_err"][0, :, 0, 1]).all() and not np.isnan(got["amplitude"][0, :, 0, 1]).any()


def test_the_neighbour_is_found_on_the_device():
    shape, N = (13, 13), 300
    cy, cx = shape[0] // 2, shape[1] // 2
    got = device_result(shape, N, 2)
    for b in range(C.B):
        miss = np.hypot(*(got["centroid_amp"][b] - (cx + C.SEPARATION, cy)))
        print("cutout %d: centroid_amp %s, %.3f px from the neighbour, offset_pix %.3f" % (b, got["centroid_amp"][b], miss, got["offset_pix"][b]))
        assert miss < np.hypot(*(got["centroid_amp"][b] - (cx, cy))) and abs(got["offset_pix"][b] - C.SEPARATION) < 0.5
        at = (b, 0, cy, cx + C.SEPARATION)
        assert abs(got["amplitude"][at] - C.NEIGHBOUR * C.A1) < 5 * got["amplitude_err"][at]


# ------------------------------------------------------------------------------------------------ statuses, frequencies, masks
@pytest.mark.parametrize("nterms", [1, 3])
def test_skipped_cutouts_frequencies_and_masks(nterms):
    shape, N = (11, 11), 129
    time, flux, err, f = C.case(shape, N, nterms)
    cubes = cubes_of(shape, N, nterms)
    whole = device_result(shape, N, nterms)
    # a skipped cutout between fitted ones: its neighbours keep their bits
    for bad in (np.nan, 0.0, -1.0):
        got = cubes.amplitude_images([f[0], bad, f[2]], nterms)
        assert list(got["status"]) == [0, 1, 0] and not got["n_used"][1].any()
        assert all(np.isnan(got[k][1]).all() for k in FLOAT_IMAGES + CENTROIDS)
        for key in whole:
            assert np.array_equal(got[key][[0, 2]], whole[key][[0, 2]], equal_nan=True), key
    # one frequency for the batch, and another unit
    one = cubes.amplitude_images(f[1], nterms)
    assert np.array_equal(one["theta"][1], whole["theta"][1], equal_nan=True) and not np.array_equal(one["theta"][2], whole["theta"][2])
    in_uhz = cubes.amplitude_images(f * 1e6 / 86400.0, nterms, freq_unit="uHz")
    print("uHz against 1/d: max |theta| difference %.3g" % max_diff(in_uhz["theta"], whole["theta"]))
    assert max_diff(in_uhz["theta"], whole["theta"]) < 1e-9 * np.nanmax(np.abs(whole["theta"]))
    # a shared and a per-cutout aperture with a corner, against the mirror
    per = C.masks(shape)
    for what, spec in (("shared mask", per[1]), ("per-cutout masks", per)):
        got = cubes.amplitude_images(f, nterms, aperture_mask=spec, column=1017, row=-33)
        ref = C.stack([PixelCube(time[b], flux[b], err[b]).amplitude_image(f[b], nterms, spec if spec.ndim == 2 else spec[b], 1017, -33)
                       for b in range(C.B)])
        check_against(got, ref, what)
        for key in FLOAT_IMAGES:
            assert np.array_equal(got[key], whole[key], equal_nan=True), key
    # a cutout without a quadratic centroid beside fitted ones
    holed = np.array(flux)
    holed[1, :, shape[0] // 2, shape[1] // 2 + C.SEPARATION - 1] = np.nan
    got = DevicePixelCubeBatch.from_arrays(time, holed, err).amplitude_images(f, nterms)
    assert list(got["status"]) == [0, 3, 0] and np.isnan(got["offset_pix"][1]) and not np.isnan(got["centroid_amp_moments"][1]).any()
    for bad in (dict(nterms=0), dict(nterms=4), dict(nterms=1.5)):
        with pytest.raises(ValueError):
            cubes.amplitude_images(f, **bad)
    with pytest.raises(ValueError):
        cubes.amplitude_images(f[:2])
    small = DevicePixelCubeBatch.from_arrays(time[:1, :4], np.ones((1, 4, 2, 5), np.float32), np.ones((1, 4, 2, 5), np.float32))
    with pytest.raises(ValueError):
        small.amplitude_images(f[0])


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("shape,N,nterms", [((13, 13), 300, 3), ((5, 7), 129, 1), ((11, 11), 7, 2)])
def test_amplitude_images_have_the_same_bits_alone_in_a_batch_and_again(shape, N, nterms):
    time, flux, err, f = C.case(shape, N, nterms)
    whole = device_result(shape, N, nterms)
    again = cubes_of(shape, N, nterms).amplitude_images(f, nterms)
    for key in whole:
        assert np.array_equal(whole[key], again[key], equal_nan=True), key
    order = [2, 1, 0]                                            # cutout 0 at position 2 and cutout 2 at position 0
    moved = DevicePixelCubeBatch.from_arrays(time[order], flux[order], err[order]).amplitude_images(f[order], nterms)
    for b in range(C.B):
        alone = DevicePixelCubeBatch.from_arrays(time[b:b + 1], flux[b:b + 1], err[b:b + 1]).amplitude_images(f[b], nterms)
        for key in whole:
            assert np.array_equal(alone[key][0], whole[key][b], equal_nan=True), (b, key)
            assert np.array_equal(moved[key][order.index(b)], whole[key][b], equal_nan=True), (b, key)


def test_resident_outputs_and_the_host_route():
    shape, N, nterms = (11, 11), 300, 2
    time, flux, err, f = C.case(shape, N, nterms)
    whole = device_result(shape, N, nterms)
    cubes = cubes_of(shape, N, nterms)
    K, npix = 2 * nterms + 1, shape[0] * shape[1]
    dev = cubes.amplitude_images(f, nterms, to_host=False)
    assert isinstance(dev["status"], np.ndarray) and np.array_equal(dev["status"], whole["status"])
    for key, n in (("theta", K), ("amplitude", nterms), ("phase", nterms), ("amplitude_err", nterms), ("snr", nterms)):
        assert isinstance(dev[key], DeviceBuffer)
        a = dev[key].download(np.float64, n * C.B * npix, stream=cubes.stream).reshape((n, C.B) + shape)     # coefficient-major
        assert np.array_equal(a.transpose(1, 0, 2, 3), whole[key], equal_nan=True), key
    for key in ("level", "chi2"):
        assert np.array_equal(dev[key].download(np.float64, C.B * npix, stream=cubes.stream).reshape((C.B,) + shape), whole[key],
                              equal_nan=True), key
    assert np.array_equal(dev["n_used"].download(np.int32, C.B * npix, stream=cubes.stream).reshape((C.B,) + shape), whole["n_used"])
    assert np.array_equal(dev["centroid_amp"][0].download(np.float64, C.B, stream=cubes.stream), whole["centroid_amp"][:, 0], equal_nan=True)
    assert np.array_equal(dev["offset"].download(np.float64, 2 * C.B, stream=cubes.stream).reshape(C.B, 2), whole["offset"], equal_nan=True)
    assert np.array_equal(dev["offset_pix"].download(np.float64, C.B, stream=cubes.stream), whole["offset_pix"], equal_nan=True)
    host = batch.amplitude_images_batch([PixelCube(time[b], flux[b], err[b]) for b in range(C.B)], f, nterms=nterms)
    for key in whole:
        assert np.array_equal(host[key], whole[key], equal_nan=True), key


# ------------------------------------------------------------------------------------------------ the chain
def test_the_chain_from_light_curves_to_amplitude_images():
    shape, N = (11, 11), 300
    cy, cx = shape[0] // 2, shape[1] // 2
    time, flux, err, f = C.case(shape, N, 1)
    cubes = DevicePixelCubeBatch.from_arrays(time[1:], flux[1:], err[1:])           # the cutouts without NaN cadences
    lcs = cubes.to_lightcurves()
    grid = np.linspace(0.5, 1.5, 401) * f[0]
    peaks = lcs.to_periodogram_peaks(grid)
    got = cubes.amplitude_images(grid, peaks=peaks)
    found = grid[peaks[:, 1].astype(int)]
    print("peak frequencies %s 1/d, planted %s" % (found, f[1:]))
    assert np.array_equal(got["frequency"], found) and np.all(np.abs(found / f[1:] - 1) < 0.01)
    assert list(got["status"]) == [0, 0]
    for b in range(2):
        assert np.hypot(*(got["centroid_amp"][b] - (cx + C.SEPARATION, cy))) < 0.5 and abs(got["offset_pix"][b] - C.SEPARATION) < 0.5
    direct = cubes.amplitude_images(found)
    for key in direct:
        assert np.array_equal(got[key], direct[key], equal_nan=True), key
    hook = lcs.to_periodogram(grid, normalization="amplitude").amplitude_images(cubes)
    assert np.array_equal(hook["frequency"], found) and np.array_equal(hook["amplitude"], direct["amplitude"], equal_nan=True)
    with pytest.raises(ValueError):
        cubes.amplitude_images(grid, peaks=peaks[:1])
