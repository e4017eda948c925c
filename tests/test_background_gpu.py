"""GPU: DevicePixelCubeBatch.estimate_background / subtract_background (csrc/pixcube.hip: cube_background_kernel,
cube_background_wide_kernel, cube_subtract_rows_kernel) against the numpy mirror PixelCube.estimate_background /
subtract_background on the cutouts of tests/background_cases.py.

Bound for everything (flux, n_pixels, scatter, mask, the subtracted cube): equal values and equal NaN positions,
``np.array_equal(..., equal_nan=True)`` on the arrays as they are — selection and one float32 subtraction are exact, so there
is no tolerance; not through a bit view, because the sign of a zero median is unspecified.

The route cut is by npix alone: cube_background_kernel (a tile of 64 cadences in LDS, one wavefront per cadence) up to
``C.ROUTE_CUT_NPIX`` = 224 pixels, cube_background_wide_kernel (one workgroup per cadence) from 225 on; ``C.CUT_SHAPES`` sit on
either side of it.
"""
import warnings

import numpy as np
import pytest

import background_cases as C
from lightkurve_amd import _capi, batch
from lightkurve_amd.device import DeviceBuffer, DevicePixelCubeBatch

pytestmark = pytest.mark.gpu

SHAPE, N, B = (11, 11), 65, 3                # the behaviour checks' batch


def equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def mirror(shape, n, b, name, first=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (create_threshold_mask's median image of an all-NaN pixel warns)
        return C.mirror(shape, n, b, name, first)


def device_flux(cubes):
    return np.stack([c.flux for c in cubes.to_host()])


def check_against_mirror(shape, n, b, names):
    dev = DevicePixelCubeBatch.from_cubes(C.cubes(shape, n, b))
    for name in names:
        spec = C.mask_spec(name, shape, b)[0]
        ref = mirror(shape, n, b, name)
        est = dev.estimate_background(spec, return_scatter=True)
        assert sorted(est) == ["flux", "mask", "n_pixels", "scatter"]
        assert est["flux"].shape == est["n_pixels"].shape == est["scatter"].shape == (b, n) and est["mask"].shape == (b,) + shape
        for key in ("mask", "n_pixels", "flux", "scatter"):
            want = np.stack([r[key] for r in ref])
            bad = np.argwhere(~((est[key] == want) | ((est[key] != est[key]) & (want != want))))
            print("%s N=%d B=%d %-10s %-8s differing values: %d" % (shape, n, b, name, key, len(bad)))
            assert equal(est[key], want), (name, key, bad[:5])
        assert "scatter" not in dev.estimate_background(spec)
        sub, info = dev.subtract_background(aperture_mask=spec, return_background=True)
        assert sub.shape == dev.shape and sub.d_time is dev.d_time and sub.d_flux_err is dev.d_flux_err
        assert sub.d_flux is not dev.d_flux and np.shares_memory(sub.time, dev.time)
        want = np.stack([r["subtracted"] for r in ref])
        got = device_flux(sub)
        print("%s N=%d B=%d %-10s subtracted differing values: %d"
              % (shape, n, b, name, int(np.sum(~((got == want) | ((got != got) & (want != want)))))))
        assert equal(got, want), name
        assert all(equal(info[key], est[key]) for key in ("flux", "n_pixels", "mask"))
        for i in range(b):
            assert sub.meta[i] == ref[i]["meta"], (name, i, sub.meta[i])
            assert "BKG_SUBTRACTED" not in dev.meta[i]


@pytest.mark.parametrize("shape", C.SHAPES)
@pytest.mark.parametrize("n", C.CADENCES)
@pytest.mark.parametrize("b", C.BATCHES)
def test_every_mask_against_the_mirror(shape, n, b):
    check_against_mirror(shape, n, b, C.MASKS)


@pytest.mark.parametrize("shape", C.CUT_SHAPES)
def test_both_sides_of_the_route_cut(shape):
    assert shape[0] * shape[1] - C.ROUTE_CUT_NPIX == (0 if shape == C.CUT_SHAPES[0] else 1)
    check_against_mirror(shape, 65, 3, C.MASKS)


def test_more_pixels_than_the_device_masks_hold():
    assert C.LARGE_SHAPE[0] * C.LARGE_SHAPE[1] > _capi.CUBE_MASK_MAX_NPIX
    check_against_mirror(C.LARGE_SHAPE, C.LARGE_N, 3, ("shared", "per cutout", "tiny", "all"))


# ------------------------------------------------------------------------------------------------ behaviour
@pytest.fixture(scope="module")
def dev():
    return DevicePixelCubeBatch.from_cubes(C.cubes(SHAPE, N, B))


@pytest.fixture(scope="module")
def fused(dev):
    return device_flux(dev.subtract_background())


@pytest.mark.parametrize("form", ["host array", "DeviceBuffer", "host dict", "device dict"])
def test_fused_equals_estimate_then_subtract(dev, fused, form):
    est = dev.estimate_background(to_host=form in ("host array", "host dict"))
    if form == "DeviceBuffer":
        assert isinstance(est["flux"], DeviceBuffer) and isinstance(est["n_pixels"], DeviceBuffer)
    given = est if form.endswith("dict") else est["flux"]
    sub, info = dev.subtract_background(background=given, return_background=True)
    assert equal(device_flux(sub), fused)
    ref = mirror(SHAPE, N, B, "background")
    assert equal(info["flux"], np.stack([r["flux"] for r in ref]))
    for i in range(B):
        want = dict(ref[i]["meta"], BKG_NPIX=ref[i]["meta"]["BKG_NPIX"] if form.endswith("dict") else -1)
        assert sub.meta[i] == want
    if form.endswith("dict"):
        assert equal(info["n_pixels"], np.stack([r["n_pixels"] for r in ref]))


def test_the_result_is_an_ordinary_batch():
    # cutouts 2 .. 4: to_lightcurves needs one number of kept cadences per batch, and the quantised cutout 1, whose 'threshold'
    # aperture reaches both infinite corners of cadence 4, loses one more than the others
    sub = DevicePixelCubeBatch.from_cubes(C.cubes(SHAPE, N, B, first=2)).subtract_background()
    ref = mirror(SHAPE, N, B, "background", first=2)
    host = C.cubes(SHAPE, N, B, first=2)
    for c, r in zip(host, ref):
        c.flux = np.array(r["subtracted"])
    twin = DevicePixelCubeBatch.from_cubes(host)
    a, b = sub.to_lightcurves("threshold"), twin.to_lightcurves("threshold")
    assert np.array_equal(a.n_off, b.n_off) and a.n_off[-1] < B * N          # the NaN-background cadences are gone
    for get in ("time_host", "flux_host", "flux_err_host"):
        assert getattr(a, get)().tobytes() == getattr(b, get)().tobytes(), get
    for method in ("moments", "quadratic"):
        ca, cb = sub.estimate_centroids(to_host=True, method=method), twin.estimate_centroids(to_host=True, method=method)
        assert ca[0].tobytes() == cb[0].tobytes() and ca[1].tobytes() == cb[1].tobytes(), method
    assert np.array_equal(sub.threshold_masks(), twin.threshold_masks())
    assert [c.meta["BKG_SUBTRACTED"] for c in sub.to_host()] == [True] * B


def test_two_runs_give_equal_bytes(dev, fused):
    again = device_flux(dev.subtract_background())
    assert again.tobytes() == fused.tobytes()
    a, b = (dev.estimate_background(return_scatter=True) for _ in range(2))
    assert all(a[key].tobytes() == b[key].tobytes() for key in a)


def test_a_cutout_does_not_depend_on_its_batch(dev, fused):
    alone = DevicePixelCubeBatch.from_cubes(C.cubes(SHAPE, N, 1, first=1))
    assert device_flux(alone.subtract_background())[0].tobytes() == fused[1].tobytes()
    inside, single = dev.estimate_background(return_scatter=True), alone.estimate_background(return_scatter=True)
    assert all(inside[key][1].tobytes() == single[key][0].tobytes() for key in inside)
    shared = C.shared_mask(SHAPE)
    a = dev.estimate_background(shared, return_scatter=True)
    b = dev.estimate_background(np.broadcast_to(shared, (B,) + SHAPE).copy(), return_scatter=True)
    assert all(a[key].tobytes() == b[key].tobytes() for key in a)
    assert (device_flux(dev.subtract_background(aperture_mask=shared)).tobytes()
            == device_flux(dev.subtract_background(aperture_mask=np.broadcast_to(shared, (B,) + SHAPE).copy())).tobytes())


def test_the_parent_cube_is_not_written(dev):
    n = int(np.prod(dev.shape))
    before = dev.d_flux.download(np.float32, n, stream=dev.stream).tobytes()
    dev.subtract_background()
    dev.subtract_background(background=np.zeros((B, N), dtype=np.float32))
    dev.synchronize()
    assert dev.d_flux.download(np.float32, n, stream=dev.stream).tobytes() == before
    assert before == np.stack([c.flux for c in C.cubes(SHAPE, N, B)]).tobytes()


def test_subtract_background_batch():
    ref = mirror(SHAPE, N, B, "background")
    out = batch.subtract_background_batch(C.cubes(SHAPE, N, B))
    assert len(out) == B
    for c, r, src in zip(out, ref, C.cubes(SHAPE, N, B)):
        assert equal(c.flux, r["subtracted"]) and c.meta == r["meta"]
        assert np.array_equal(c.flux_err, src.flux_err) and np.array_equal(c.time, src.time)
    resident = batch.subtract_background_batch(C.cubes(SHAPE, N, B), aperture_mask="all", to_host=False)
    assert isinstance(resident, DevicePixelCubeBatch)
    assert equal(device_flux(resident), np.stack([r["subtracted"] for r in mirror(SHAPE, N, B, "all")]))


def test_errors(dev):
    with pytest.raises(ValueError):
        dev.estimate_background(np.ones((SHAPE[0], SHAPE[1] + 1), dtype=bool))
    with pytest.raises(ValueError):
        dev.subtract_background(aperture_mask=np.ones((B + 1,) + SHAPE, dtype=bool))
    with pytest.raises(ValueError):
        dev.subtract_background(background=np.zeros((B, N + 1), dtype=np.float32))
    with pytest.raises(ValueError):
        dev.subtract_background(background=np.zeros(N, dtype=np.float32))
    with pytest.raises(ValueError):
        dev.estimate_background("pipeline")
    with pytest.raises(ValueError):
        dev.subtract_background(aperture_mask="pipeline")
