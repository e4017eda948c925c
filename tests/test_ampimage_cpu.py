"""CPU: PixelCube.amplitude_image, the numpy mirror of the resident amplitude images, against ls_model_host pixel by pixel and
against the scene that tests/ampimage_cases.py plants.

ls_model_host refers its phases to the first time it is given, the pixel's own first cadence; the mirror refers every pixel to
the cutout's t_ref.  The comparison therefore turns each harmonic of ls_model_host's (sin, cos) pair by m w (t_first - t_ref), a
rotation that changes neither the level, the amplitude nor chi2.

Bounds: theta, level and chi2 within 1e-11 of the image's largest finite |value| (two float64 solves of the same well-
conditioned system); counts, statuses and NaN patterns exact."""
import numpy as np
import pytest

import ampimage_cases as C
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.periodogram import ls_model_host

FLOAT_IMAGES = ("theta", "level", "amplitude", "phase", "amplitude_err", "snr", "chi2")


def per_pixel_reference(time, flux, f, nterms):
    """ls_model_host of every pixel on its own cadences -> theta (K, ny, nx) referred to the first finite time, level, chi2,
    n_used."""
    N, ny, nx = flux.shape
    K = 2 * nterms + 1
    fin = np.isfinite(time)
    t_ref = time[fin][0]
    theta, level, chi2 = np.full((K, ny, nx), np.nan), np.full((ny, nx), np.nan), np.full((ny, nx), np.nan)
    n_used = np.zeros((ny, nx), dtype=np.int32)
    for iy in range(ny):
        for ix in range(nx):
            y = flux[:, iy, ix].astype(np.float64)
            ok = fin & ~np.isnan(y)
            n_used[iy, ix] = ok.sum()
            if not ok.any():
                continue
            res = ls_model_host(time[ok], y[ok], None, f, nterms, singular="nan")
            th = res["theta"].copy()
            for m in range(1, nterms + 1):
                a = 2 * np.pi * m * f * (time[ok][0] - t_ref)
                s, c = res["theta"][2 * m - 1], res["theta"][2 * m]
                th[2 * m - 1], th[2 * m] = s * np.cos(a) + c * np.sin(a), c * np.cos(a) - s * np.sin(a)
            theta[:, iy, ix], level[iy, ix], chi2[iy, ix] = th, res["y_mean"] + res["theta"][0], res["chi2_model"]
    return theta, level, chi2, n_used


def scaled_diff(a, b):
    ok = np.isfinite(b)
    return float(np.max(np.abs(a[ok] - b[ok])) / np.max(np.abs(b[ok]))) if ok.any() else 0.0


@pytest.mark.parametrize("nterms", [1, 2, 3])
@pytest.mark.parametrize("N", C.NS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_mirror_equals_ls_model_host_per_pixel(shape, N, nterms):
    time, flux, err, f = C.case(shape, N, nterms)
    got = C.mirror(shape, N, nterms)
    K = 2 * nterms + 1
    for b in (0, 1):
        valid = int(np.isfinite(time[b]).sum())
        if valid < K + 1:
            assert got["status"][b] == 2 and not got["n_used"][b].any(), (b, got["status"][b])
            assert all(np.isnan(got[k][b]).all() for k in FLOAT_IMAGES), b
            continue
        theta, level, chi2, n_used = per_pixel_reference(time[b], flux[b], f[b], nterms)
        # (in the 3 x 3 cutout 0 the NaN pixels of the first row are inside the only patch: no quadratic centroid)
        assert got["status"][b] == (3 if shape == (3, 3) and b == 0 else 0) and got["t_ref"][b] == time[b][np.isfinite(time[b])][0]
        assert np.isnan(got["offset_pix"][b]) == (got["status"][b] == 3)
        assert np.array_equal(got["n_used"][b], n_used), b
        for key, ref in (("theta", theta), ("level", level), ("chi2", chi2)):
            assert np.array_equal(np.isnan(got[key][b]), np.isnan(ref)), (b, key)
            d = scaled_diff(got[key][b], ref)
            print("%s N=%d nterms=%d cutout %d %s: max |mirror - ls_model_host| / max |image| = %.3g" % (shape, N, nterms, b, key, d))
            assert d < 1e-11, (b, key, d)


@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_nan_patterns_and_counts(nterms):
    shape, N = (5, 7), 300
    time, flux, err, f = C.case(shape, N, nterms)
    got = C.mirror(shape, N, nterms)
    K = 2 * nterms + 1
    usable = N - len(C.nan_times(N)) - 1                       # finite time, not the whole-NaN cadence
    n = got["n_used"][0]
    assert n.dtype == np.int32 and n[0, 0] == 0 and n[0, 1] == K and n[0, 2] == K - 1 and n[2, 3] == usable
    assert 0.8 * usable < n[1, 0] < usable
    assert (got["n_used"][1] == N).all() and got["theta"].shape == (C.B, K) + shape and got["amplitude"].shape == (C.B, nterms) + shape
    nan_all = np.zeros(shape, dtype=bool)
    nan_all[0, 0] = nan_all[0, 2] = True                        # no value; fewer than K values
    for key in FLOAT_IMAGES:
        im = got[key][0].reshape((-1,) + shape)
        expect = nan_all.copy()
        if key in ("amplitude_err", "snr"):
            expect[0, 1] = True                                 # exactly K values: a fit, no degrees of freedom left
        assert all(np.array_equal(np.isnan(layer), expect) for layer in im), key
        assert not np.isnan(got[key][1]).any(), key
    assert got["chi2"][0, 0, 1] < 1e-12 * np.nanmax(got["chi2"][0])      # the exactly determined fit leaves no residual
    assert list(got["status"]) == [0, 0, 0]


def test_statuses():
    shape, N = (5, 7), 129
    time, flux, err, f = C.case(shape, N, 1)
    cube = PixelCube(time[0], flux[0], err[0])
    for bad in (np.nan, 0.0, -3.0, np.inf):
        out = cube.amplitude_image(bad)
        assert out["status"] == 1 and not out["n_used"].any()
        assert all(np.isnan(out[k]).all() for k in FLOAT_IMAGES + ("centroid_amp", "centroid_level_moments", "offset", "offset_pix"))
    for nterms, n_finite, status in ((1, 3, 2), (1, 4, 0), (3, 7, 2), (3, 8, 0)):      # K + 1 cadences with a finite time
        t = time[1].copy()
        t[n_finite:] = np.nan
        out = PixelCube(t, flux[1], err[1]).amplitude_image(0.11 / C.CADENCE, nterms)      # a handful of cadences round one cycle
        assert out["status"] == status, (nterms, n_finite, out["status"])
        assert np.isnan(out["level"]).all() == (status == 2) and (out["n_used"] == (n_finite if status == 0 else 0)).all()
    # a pixel without a value beside the brightest amplitude: the quadratic patch holds a NaN
    ny, nx = shape
    holed = flux[1].copy()
    holed[:, ny // 2, nx // 2 + C.SEPARATION - 1] = np.nan
    out = PixelCube(time[1], holed, err[1]).amplitude_image(f[1])
    assert out["status"] == 3 and np.isnan(out["centroid_amp"]).all() and np.isnan(out["offset_pix"])
    assert not np.isnan(out["centroid_amp_moments"]).any()
    assert PixelCube(time[1], flux[1], err[1]).amplitude_image(f[1])["status"] == 0


@pytest.mark.parametrize("shape", [(11, 11), (13, 13)])
@pytest.mark.parametrize("nterms", [1, 2, 3])
def test_the_planted_neighbour_is_recovered(shape, nterms):
    N = 300
    ny, nx = shape
    cy, cx = ny // 2, nx // 2
    got = C.mirror(shape, N, nterms)
    for b in range(C.B):
        amp, err, phase = got["amplitude"][b, 0, cy, cx + C.SEPARATION], got["amplitude_err"][b, 0, cy, cx + C.SEPARATION], \
            got["phase"][b, 0, cy, cx + C.SEPARATION]
        planted = C.NEIGHBOUR * C.A1                              # the neighbour's brightest pixel is its centre
        dphi = (phase - C.PHI1 + np.pi) % (2 * np.pi) - np.pi
        print("%s nterms=%d cutout %d: amplitude %.3f +- %.3f (planted %.3f), phase off by %.4f rad (1 sigma %.4f)"
              % (shape, nterms, b, amp, err, planted, dphi, err / amp))
        assert abs(amp - planted) < 5 * err and abs(dphi) < 5 * err / amp
        assert got["snr"][b, 0, cy, cx + C.SEPARATION] == amp / err
        to_neighbour = np.hypot(*(got["centroid_amp"][b] - (cx + C.SEPARATION, cy)))
        to_target = np.hypot(*(got["centroid_amp"][b] - (cx, cy)))
        print("    centroid_amp %s, offset_pix %.3f" % (got["centroid_amp"][b], got["offset_pix"][b]))
        assert to_neighbour < to_target and abs(got["offset_pix"][b] - C.SEPARATION) < 0.5
        assert np.allclose(got["offset"][b], got["centroid_amp"][b] - got["centroid_level"][b], atol=0, rtol=0)
        if nterms >= 2:
            assert abs(got["amplitude"][b, 1, cy, cx + C.SEPARATION] - C.NEIGHBOUR * C.A2) < 5 * got["amplitude_err"][b, 1, cy, cx + C.SEPARATION]


def test_masks_and_origin():
    shape, N = (11, 11), 128
    time, flux, err, f = C.case(shape, N, 1)
    cube = PixelCube(time[1], flux[1], err[1])
    plain = cube.amplitude_image(f[1])
    left = np.zeros(shape, dtype=bool)
    left[:, :shape[1] // 2 + 2] = True                           # the neighbour's core is outside: the target's own pixels win
    out = cube.amplitude_image(f[1], aperture_mask=left, column=200, row=100)
    assert np.array_equal(out["amplitude"], plain["amplitude"])
    assert np.allclose(out["centroid_level"], plain["centroid_level"] + (200, 100), atol=1e-9)
    assert out["centroid_amp"][0] - 200 < shape[1] // 2 + 2 and out["offset_pix"] < plain["offset_pix"]


def test_arguments():
    time, flux, err, f = C.case((5, 7), 7, 1)
    cube = PixelCube(time[1], flux[1], err[1])
    for bad in (0, 4, 1.5):
        with pytest.raises(ValueError):
            cube.amplitude_image(f[1], nterms=bad)
    with pytest.raises(ValueError):
        cube.amplitude_image(f)                                   # one frequency per cutout
    with pytest.raises(ValueError):
        cube.amplitude_image([f[1]])
    with pytest.raises(ValueError):
        PixelCube(time[1], flux[1][:, :2], err[1][:, :2]).amplitude_image(f[1])      # 2 x 7: no 3 x 3 patch
    with pytest.raises(ValueError):
        cube.amplitude_image(f[1], aperture_mask=np.ones((3, 3), dtype=bool))
