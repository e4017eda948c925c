"""GPU: estimate_centroids(method="quadratic") and the resident transit difference images (csrc/pixcube.hip:
cube_centroids_quadratic_kernel, cube_diffimage_*_kernel, image_centroids_kernel) against the numpy restatement of
tests/diffimage_cases.py.

Bounds: peaks, class bytes, counts, statuses and NaN patterns exact; centroids and offsets 1e-9 px (the house rule; the
restatement's np.linalg.inv fit matrix and the kernel's integer table differ by 1e-14 px on these frames); images 1e-9 of the
image's largest finite |value| (float64 sums of at most a few hundred float32 values in another order: ~1e-15).  Every
comparison prints its largest difference before it asserts.
"""
import functools

import numpy as np
import pytest

import diffimage_cases as C
from lightkurve_amd import batch
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.device import DeviceBuffer, DeviceLightCurveBatch, DevicePixelCubeBatch

pytestmark = pytest.mark.gpu

IMAGES = ("mean_in", "mean_out", "diff", "diff_err")
CENTROIDS = ("centroid_diff", "centroid_out", "centroid_diff_moments", "centroid_out_moments", "offset", "offset_pix")


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def max_diff(a, b):
    ok = ~np.isnan(np.asarray(b, dtype=np.float64))
    return float(np.max(np.abs(np.asarray(a)[ok] - np.asarray(b)[ok]))) if ok.any() else 0.0


def centroid_cubes(shape):
    flux = C.centroid_frames(shape)
    return DevicePixelCubeBatch.from_arrays(np.tile(C.times(C.N_CENTROID), (3, 1)), flux, np.ones_like(flux))


# ------------------------------------------------------------------------------------------------ quadratic centroids
@pytest.mark.parametrize("shape", C.SHAPES)
@pytest.mark.parametrize("masks", ["all", "shared", "per cutout"])
def test_quadratic_centroids(shape, masks):
    flux = C.centroid_frames(shape)
    cubes = centroid_cubes(shape)
    per = C.cutout_masks(shape)
    spec = {"all": "all", "shared": C.partial_mask(shape), "per cutout": per}[masks]
    column, row = (0, 0) if masks == "all" else (1017, -33)
    col, rw, peak = cubes.estimate_centroids(aperture_mask=spec, column=column, row=row, to_host=True, method="quadratic",
                                             return_peak=True)
    assert col.shape == rw.shape == peak.shape == (3, C.N_CENTROID) and peak.dtype == np.int32
    worst = 0.0
    for b in range(3):
        m = None if masks == "all" else spec if masks == "shared" else per[b]
        rc, rr, rp = C.centroids_quadratic(flux[b], m, column, row)
        assert np.array_equal(peak[b], rp), (b, np.flatnonzero(peak[b] != rp))
        assert same_nan(col[b], rc) and same_nan(rw[b], rr), b
        worst = max(worst, max_diff(col[b], rc), max_diff(rw[b], rr))
    print("%s, mask %s: max |device - restatement| = %.3g px" % (shape, masks, worst))
    assert worst < 1e-9
    # what the special frames of cutout 0 are for
    nan = np.isnan(col[0]) & np.isnan(rw[0])
    assert nan[[C.NAN_INSIDE, C.ALL_NAN]].all() and peak[0, C.ALL_NAN] == -1
    if masks == "all":
        assert nan[C.CONSTANT]                              # det = 0
        assert peak[0, C.TWO_MAXIMA] == 1 and peak[0, C.CORNER] == shape[0] * shape[1] - 1
        assert not nan[[C.TWO_MAXIMA, C.CORNER, C.EDGE, C.NAN_OUTSIDE]].any()
    else:
        assert peak[0, C.NEGATIVE] == 0                    # the masked-out zero at pixel 0 beats the all-negative aperture
        assert nan[C.NEGATIVE] or shape == (3, 3)          # ... and its patch is flat where it lies outside the mask
    # the default stays the moments, bit for bit, and two outputs
    d_c, d_r = cubes.estimate_centroids(aperture_mask=spec, column=column, row=row)
    mc, mr = cubes.estimate_centroids(aperture_mask=spec, column=column, row=row, to_host=True, method="moments")
    assert np.array_equal(d_c.download(np.float64, 3 * C.N_CENTROID, stream=cubes.stream).reshape(3, -1), mc, equal_nan=True)


def test_quadratic_centroid_buffers_feed_sff_correct():
    shape = (7, 9)
    rng = np.random.RandomState(5)
    B, N = 2, C.N_CENTROID
    flux = np.stack([[C.psf(shape, 4 + rng.uniform(-0.5, 0.5), 3 + rng.uniform(-0.5, 0.5)) + 20 + rng.normal(0, 3, shape)
                      for _ in range(N)] for _ in range(B)]).astype(np.float32)
    cubes = DevicePixelCubeBatch.from_arrays(np.tile(C.times(N), (B, 1)), flux, np.full_like(flux, 3.0))
    d_col, d_row = cubes.estimate_centroids(column=5, row=15, method="quadratic")
    assert isinstance(d_col, DeviceBuffer) and isinstance(d_row, DeviceBuffer)
    res = cubes.to_lightcurves().sff_correct(d_col, d_row, window_points=[[N // 2]] * B, bins=5, degree=3, timescale=0.5)
    print("sff_correct on quadratic centroids: status", list(res["status"]))
    assert len(res["status"]) == B
    with pytest.raises(ValueError):
        cubes.estimate_centroids(method="psf")
    with pytest.raises(ValueError):
        cubes.estimate_centroids(method="moments", return_peak=True)
    small = DevicePixelCubeBatch.from_arrays(np.tile(C.times(4), (1, 1)), np.ones((1, 4, 2, 5), np.float32), np.ones((1, 4, 2, 5), np.float32))
    with pytest.raises(ValueError):
        small.estimate_centroids(method="quadratic")                 # no 3 x 3 patch


# ------------------------------------------------------------------------------------------------ difference images
def boxes():
    P, t0, D = (np.array(v) for v in zip(*C.BOXES))
    return P, t0, D


@functools.lru_cache(maxsize=None)
def device_result(shape, dip_on="neighbour"):
    """difference_images of the three cutouts of C.diff_case in one batch; shared, read-only."""
    time, flux, err = C.diff_case(shape, dip_on)
    P, t0, D = boxes()
    return DevicePixelCubeBatch.from_arrays(time, flux, err).difference_images(P, t0, D)


def check_against(got, ref, what):
    for key in ("cadence_class", "n_in", "n_out", "status"):
        assert np.array_equal(got[key], ref[key]), (what, key)
    for key in IMAGES:
        assert same_nan(got[key], ref[key]), (what, key)
        for b in range(len(ref[key])):
            if np.isnan(ref[key][b]).all():
                continue
            err = max_diff(got[key][b], ref[key][b]) / np.nanmax(np.abs(ref[key][b]))
            print("%s cutout %d %s: max |device - restatement| / max |image| = %.3g" % (what, b, key, err))
            assert err < 1e-9, (what, key, b)
    for key in CENTROIDS:
        assert same_nan(got[key], ref[key]), (what, key)
        err = max_diff(got[key], ref[key])
        print("%s %s: max |device - restatement| = %.3g px" % (what, key, err))
        assert err < 1e-9, (what, key)


@pytest.mark.parametrize("shape", C.DIFF_SHAPES)
def test_difference_images_against_restatement(shape):
    got, ref = device_result(shape), C.diff_reference(shape)
    assert got["mean_in"].shape == (3,) + shape and got["centroid_diff"].shape == (3, 2) and got["offset_pix"].shape == (3,)
    assert got["n_in"].dtype == np.int32 and 20 <= got["n_in"][0] <= 60 and got["n_out"][0] > 1.5 * got["n_in"][0]
    check_against(got, ref, str(shape))
    assert list(got["status"]) == [0, 0, 1] and got["n_in"][2] == 0
    assert all(np.isnan(got[k][2]).all() for k in ("mean_in", "diff", "diff_err", "centroid_diff", "offset"))
    # pixel (0, 0) has no in-transit value, pixel (0, 1) some
    assert np.isnan(got["mean_in"][0, 0, 0]) and np.isnan(got["diff"][0, 0, 0]) and not np.isnan(got["mean_out"][0, 0, 0])
    assert not np.isnan(got["diff"][0, 0, 1])


@pytest.mark.parametrize("shape", C.DIFF_SHAPES)
def test_difference_image_finds_the_dimming_pixel(shape):
    cy, cx = shape[0] // 2, shape[1] // 2
    got = device_result(shape, "neighbour")
    miss = np.hypot(got["centroid_diff"][0, 0] - (cx + 2), got["centroid_diff"][0, 1] - cy)
    print("neighbour dips: centroid_diff %s, %.3f px from the neighbour, offset_pix %.3f" % (got["centroid_diff"][0], miss, got["offset_pix"][0]))
    assert miss < 0.2 and got["offset_pix"][0] > 1.5
    got = device_result(shape, "target")
    print("target dips: centroid_diff %s, offset_pix %.3f" % (got["centroid_diff"][0], got["offset_pix"][0]))
    assert got["offset_pix"][0] < 0.2


@pytest.mark.parametrize("shape", C.DIFF_SHAPES)
def test_difference_images_have_the_same_bits_alone_in_a_batch_and_again(shape):
    time, flux, err = C.diff_case(shape)
    P, t0, D = boxes()
    whole = device_result(shape)
    again = DevicePixelCubeBatch.from_arrays(time, flux, err).difference_images(P, t0, D)
    for key in whole:
        assert np.array_equal(whole[key], again[key], equal_nan=True), key
    for b in range(3):
        alone = DevicePixelCubeBatch.from_arrays(time[b:b + 1], flux[b:b + 1], err[b:b + 1]).difference_images(P[b], t0[b], D[b])
        for key in whole:
            assert np.array_equal(alone[key][0], whole[key][b], equal_nan=True), (b, key)


def test_difference_images_other_routes_and_arguments():
    shape = (7, 9)
    time, flux, err = C.diff_case(shape)
    P, t0, D = boxes()
    whole = device_result(shape)
    cubes = DevicePixelCubeBatch.from_arrays(time, flux, err)
    # resident outputs: DeviceBuffers, only counts and statuses on the host
    dev = cubes.difference_images(P, t0, D, to_host=False)
    for key in ("n_in", "n_out", "status"):
        assert isinstance(dev[key], np.ndarray) and np.array_equal(dev[key], whole[key])
    for key in IMAGES:
        assert np.array_equal(dev[key].download(np.float64, whole[key].size, stream=cubes.stream).reshape(whole[key].shape), whole[key],
                              equal_nan=True), key
    assert np.array_equal(dev["centroid_diff"][0].download(np.float64, 3, stream=cubes.stream), whole["centroid_diff"][:, 0], equal_nan=True)
    assert np.array_equal(dev["offset"].download(np.float64, 6, stream=cubes.stream).reshape(3, 2), whole["offset"], equal_nan=True)
    # a mask, a corner and other widths, against the restatement
    mask = np.zeros(shape, dtype=bool)
    mask[1:6, 2:9] = True
    got = cubes.difference_images(P, t0, D, in_width=0.4, out_inner=1.2, out_outer=2.5, aperture_mask=mask, column=200, row=100)
    one = [C.difference_image(time[b], flux[b], err[b], P[b], t0[b], D[b], 0.4, 1.2, 2.5, mask, 200, 100) for b in range(3)]
    check_against(got, {k: np.stack([np.asarray(o[k]) for o in one]) for k in one[0]}, "masked")
    # the host list route and the BLS result's hook give the resident call's bits
    host = batch.difference_images_batch([PixelCube(time[b], flux[b], err[b]) for b in range(3)], P, t0, D)
    for key in whole:
        assert np.array_equal(host[key], whole[key], equal_nan=True), key
    t = C.times(C.N_DIFF)
    lcs = DeviceLightCurveBatch.from_arrays(np.tile(t, 3), np.nansum(flux, axis=(2, 3)).astype(np.float64).ravel(),
                                            np.ones(3 * C.N_DIFF), np.arange(4, dtype=np.int64) * C.N_DIFF)
    res = lcs.bls(np.linspace(2.0, 4.0, 40), duration=[0.1, 0.2])
    hook = res.difference_images(cubes, period=P, duration=D, transit_time=t0)
    for key in whole:
        assert np.array_equal(hook[key], whole[key], equal_nan=True), key
    peak = res.difference_images(cubes)                                     # every target's own peak
    pk = res.peaks()
    direct = cubes.difference_images(pk["period"], pk["transit_time"], pk["duration"])
    assert all(np.array_equal(peak[key], direct[key], equal_nan=True) for key in whole)
    with pytest.raises(ValueError):
        res.difference_images(DevicePixelCubeBatch.from_arrays(time[:2], flux[:2], err[:2]))
    for bad in (dict(in_width=0.0), dict(in_width=1.5), dict(out_inner=2.0), dict(out_outer=0.9)):
        with pytest.raises(ValueError):
            cubes.difference_images(P, t0, D, **bad)
    with pytest.raises(ValueError):
        cubes.difference_images([3.1, 0.0, 2.0], t0, D)
    with pytest.raises(ValueError):
        cubes.difference_images(P[:2], t0, D)
