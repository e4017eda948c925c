"""GPU: the resident per-pixel periodograms (csrc/pixelpg.hip: cube_pixelpg_stats_kernel, cube_pixelpg_spectra_kernel<false, 2> and
<true, 1>, cube_pixelpg_peaks_kernel) against the numpy mirror PixelCube.pixel_periodogram on the cases of
tests/pixelpg_cases.py.

Bounds: status, n_used, NaN patterns and shapes exact; power within 1e-9 of each pixel spectrum's largest finite value (the
house rule for float64 sums in another order); peak_index equal to the mirror's wherever the mirror's two largest powers differ
by more than 1e-6 of the largest, elsewhere peak_power within the same 1e-9 — and those excused pixels are at most 1 % of all
(tests/test_pixelpg_cpu.py asserts that of the mirror alone); peak_power has the bits of power at peak_index and peak_frequency
is the grid value.  Every comparison prints its largest difference before it asserts.  Every test here fails without
DevicePixelCubeBatch.pixel_periodograms and lk_cube_pixel_ls_batch_dev."""
import functools

import numpy as np
import pytest

import pixelpg_cases as C
from lightkurve_amd import batch
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.device import DeviceBuffer, DevicePixelCubeBatch

pytestmark = pytest.mark.gpu

KEYS = ("power", "peak_power", "peak_index", "peak_frequency", "n_used", "status", "t_ref", "frequency")
UHZ = C.UHZ_PER_CPD


def cubes_of(shape, N):
    return DevicePixelCubeBatch.from_arrays(*C.case(shape, N))


def grid_in(N, normalization, F=None):
    return C.grid(N, F) * (UHZ if normalization == "psd" else 1.0)


@functools.lru_cache(maxsize=None)
def device_result(shape, N, normalization="amplitude", F=None):
    """pixel_periodograms of the three cutouts of C.case in one batch; shared, read-only."""
    return cubes_of(shape, N).pixel_periodograms(grid_in(N, normalization, F), normalization)


def check_own_peaks(got):
    """peak_power has the bits of power at peak_index, peak_frequency is the grid value, -1 / NaN without a finite power."""
    power, idx = got["power"], got["peak_index"]
    assert idx.dtype == np.int32 and got["n_used"].dtype == np.int32 and got["status"].dtype == np.int32
    found = idx >= 0
    assert np.array_equal(found, (~np.isnan(power)).any(axis=-3))
    at = np.take_along_axis(power, np.expand_dims(np.clip(idx, 0, None), -3), axis=-3).squeeze(-3)
    assert np.array_equal(got["peak_power"], np.where(found, at, np.nan), equal_nan=True)
    assert np.array_equal(got["peak_frequency"], np.where(found, got["frequency"][np.clip(idx, 0, None)], np.nan), equal_nan=True)
    top = np.max(np.where(np.isnan(power), -np.inf, power), axis=-3)
    assert np.array_equal(at[found], top[found])                 # the largest, and (argmax of the device's own power) the first
    assert np.array_equal(idx[found], np.argmax(np.where(np.isnan(power), -np.inf, power), axis=-3)[found])


def check_against(got, ref, what):
    """-> (excused, pixels): the pixels whose peak_index may differ, and all pixels with a spectrum."""
    assert set(got) == set(KEYS), what
    for key in ("status", "n_used"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], ref[key]), (what, key)
    assert np.array_equal(got["t_ref"], ref["t_ref"], equal_nan=True) and np.array_equal(got["frequency"], ref["frequency"])
    for key in ("power", "peak_power", "peak_frequency", "peak_index"):
        assert got[key].shape == ref[key].shape, (what, key)
    assert np.array_equal(np.isnan(got["power"]), np.isnan(ref["power"])), what
    assert np.array_equal(np.isnan(got["peak_power"]), np.isnan(ref["peak_power"])), what
    top = np.max(np.where(np.isnan(ref["power"]), -np.inf, ref["power"]), axis=-3)            # (B, ny, nx)
    has = np.isfinite(top)
    with np.errstate(invalid="ignore"):
        rel = np.abs(got["power"] - ref["power"]) / np.expand_dims(top, -3)
        rel_peak = np.abs(got["peak_power"] - ref["peak_power"]) / top
    err = float(np.nanmax(rel)) if has.any() else 0.0
    print("%s power: max |device - mirror| / max of the pixel's spectrum = %.3g over %d pixels" % (what, err, has.sum()))
    assert err < 1e-9, what
    gap = C.top_two_gap(ref["power"])
    clear = has & ~(gap <= 1e-6)                                  # (a spectrum of one frequency has no second power: clear)
    excused = has & ~clear
    wrong = clear & (got["peak_index"] != ref["peak_index"])
    print("%s peak_index: %d of %d clear pixels differ, %d excused; peak_power max rel %.3g"
          % (what, wrong.sum(), clear.sum(), excused.sum(), float(np.nanmax(rel_peak)) if has.any() else 0.0))
    assert not wrong.any(), what
    assert np.array_equal(got["peak_index"][~has], ref["peak_index"][~has]) and (ref["peak_index"][~has] == -1).all()
    assert not has.any() or float(np.nanmax(rel_peak)) < 1e-9, what
    check_own_peaks(got)
    return int(excused.sum()), int(has.sum())


# ------------------------------------------------------------------------------------------------ device against the mirror
AGAINST = [(shape, N, "amplitude") for shape in C.SHAPES for N in C.NS] + [((5, 7), 128, "psd"), ((5, 7), 300, "psd")]
TALLY = {}


@pytest.mark.parametrize("shape,N,normalization", AGAINST)
def test_pixel_periodograms_against_the_mirror(shape, N, normalization):
    got, ref = device_result(shape, N, normalization), C.mirror(shape, N, normalization)
    assert got["power"].shape == (C.B, C.n_freq(N)) + shape and got["peak_index"].shape == (C.B,) + shape
    TALLY[(shape, N, normalization)] = check_against(got, ref, "%s N=%d %s" % (shape, N, normalization))
    n = got["n_used"][0]                                         # what the special pixels of cutout 0 are for
    assert n[0, 0] == 0 and n[0, 1] == 3 and n[0, 2] == 2 and 4 <= n[1, 0] <= n[1, 1]
    assert np.isnan(got["power"][0, :, 0, :3]).all() and (got["peak_index"][0, 0, :3] == -1).all()
    assert not np.isnan(got["power"][1:]).any() and not np.isnan(got["power"][0, :, 1, 0]).any()


def test_the_excused_pixels_are_few():
    """Over every case of the test above (run here where it has not run yet)."""
    for shape, N, normalization in AGAINST:
        if (shape, N, normalization) not in TALLY:
            TALLY[(shape, N, normalization)] = check_against(device_result(shape, N, normalization), C.mirror(shape, N, normalization),
                                                              "%s N=%d %s" % (shape, N, normalization))
    excused, pixels = (sum(v[i] for v in TALLY.values()) for i in (0, 1))
    print("%d of %d pixels are excused from the peak_index comparison" % (excused, pixels))
    assert pixels > 4000 and excused <= 0.01 * pixels


@pytest.mark.parametrize("F", C.TILE_FS)
def test_the_frequency_tile_grids(F):
    shape, N = C.TILE_CASE
    got, ref = device_result(shape, N, "amplitude", F), C.mirror(shape, N, "amplitude", F)
    assert got["power"].shape == (C.B, F) + shape
    excused, pixels = check_against(got, ref, "F=%d" % F)
    assert excused <= 0.01 * pixels


# ------------------------------------------------------------------------------------------------ outputs
def test_peak_images_alone_and_resident_outputs():
    shape, N = (13, 13), 300
    whole = device_result(shape, N)
    cubes = cubes_of(shape, N)
    F, npix = C.n_freq(N), shape[0] * shape[1]
    alone = cubes.pixel_periodograms(C.grid(N), return_power=False)
    assert set(alone) == set(KEYS) - {"power"}
    for key in alone:
        assert np.array_equal(alone[key], whole[key], equal_nan=True), key
    for return_power in (True, False):
        dev = cubes.pixel_periodograms(C.grid(N), return_power=return_power, to_host=False)
        assert isinstance(dev["status"], np.ndarray) and np.array_equal(dev["status"], whole["status"])
        assert ("power" in dev) == return_power and "peak_frequency" not in dev
        assert np.array_equal(dev["t_ref"], whole["t_ref"]) and np.array_equal(dev["frequency"], whole["frequency"])
        for key, dtype in (("peak_power", np.float64), ("peak_index", np.int32), ("n_used", np.int32)):
            assert isinstance(dev[key], DeviceBuffer)
            a = dev[key].download(dtype, C.B * npix, stream=cubes.stream).reshape((C.B,) + shape)
            assert np.array_equal(a, whole[key], equal_nan=True), key
        if return_power:
            a = dev["power"].download(np.float64, C.B * F * npix, stream=cubes.stream).reshape((C.B, F) + shape)   # [B][F][npix]
            assert np.array_equal(a, whole["power"], equal_nan=True)


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("shape,N", [((13, 13), 300), ((5, 7), 129)])
def test_the_same_bits_alone_in_a_batch_reversed_and_again(shape, N):
    time, flux, err = C.case(shape, N)
    whole = device_result(shape, N)
    again = cubes_of(shape, N).pixel_periodograms(C.grid(N))
    order = [2, 1, 0]
    moved = DevicePixelCubeBatch.from_arrays(time[order], flux[order], err[order]).pixel_periodograms(C.grid(N))
    for b in range(C.B):                                         # cutout 1 and the two others
        alone = DevicePixelCubeBatch.from_arrays(time[b:b + 1], flux[b:b + 1], err[b:b + 1]).pixel_periodograms(C.grid(N))
        for key in KEYS:
            if key == "frequency":
                assert np.array_equal(alone[key], whole[key]) and np.array_equal(again[key], whole[key])
                continue
            assert np.array_equal(again[key][b], whole[key][b], equal_nan=True), (b, key)
            assert np.array_equal(alone[key][0], whole[key][b], equal_nan=True), (b, key)
            assert np.array_equal(moved[key][order.index(b)], whole[key][b], equal_nan=True), (b, key)


@pytest.mark.parametrize("shape,N", [((13, 13), 300), ((11, 11), 129), ((3, 3), 20)])
def test_cutouts_without_any_nan_against_the_mirror(shape, N):
    """The path without the correction must be right on its own: nan_to_num of the flux, finite times."""
    time, flux, err = C.case(shape, N)
    time = 1000.25 + np.arange(N) * C.CADENCE + np.zeros((C.B, 1))
    flux = np.nan_to_num(flux, nan=1e4).astype(np.float32)
    got = DevicePixelCubeBatch.from_arrays(time, flux, err).pixel_periodograms(C.grid(N))
    ref = C.stack([PixelCube(time[b], flux[b], err[b]).pixel_periodogram(C.grid(N)) for b in range(C.B)])
    ref["frequency"] = C.grid(N)
    assert (got["n_used"] == N).all() and not np.isnan(got["power"][:, :, 1:]).any()
    excused, pixels = check_against(got, ref, "no NaN %s N=%d" % (shape, N))
    assert excused <= 0.01 * pixels


# ------------------------------------------------------------------------------------------------ the science check
def test_the_neighbour_is_found_at_its_frequency():
    import ampimage_cases as A
    shape, N = (13, 13), 300
    cy, cx = shape[0] // 2, shape[1] // 2
    got = device_result(shape, N)
    planted = A.frequencies(N)
    for b in range(C.B):
        nearest = got["frequency"][np.argmin(np.abs(got["frequency"] - planted[b]))]
        at = (b, cy, cx + A.SEPARATION)
        print("cutout %d: neighbour peaks at %.4f 1/d (planted %.4f, nearest grid value %.4f), peak_power %.3f; the star's centre %.3f"
              % (b, got["peak_frequency"][at], planted[b], nearest, got["peak_power"][at], got["peak_power"][b, cy, cx]))
        assert got["peak_frequency"][at] == nearest
        assert got["peak_power"][b, cy, cx] <= got["peak_power"][at]


# ------------------------------------------------------------------------------------------------ errors, statuses, the host route
def test_errors_a_cutout_without_times_and_the_host_route():
    shape, N = (11, 11), 129
    time, flux, err = C.case(shape, N)
    cubes = cubes_of(shape, N)
    whole = device_result(shape, N)
    g = C.grid(N)
    for bad in (np.r_[0.0, g], np.r_[g[:3], np.nan, g[3:]], np.r_[-g[0], g]):
        with pytest.raises(ValueError):
            cubes.pixel_periodograms(bad)
    with pytest.raises(ValueError):
        cubes.pixel_periodograms(g, normalization="standard")
    with pytest.raises(ValueError) as too_large:
        cubes.pixel_periodograms(g, max_output_mb=0.05)           # the cube of 3 x 37 x 121 float64 is 0.1 MiB
    assert "return_power=False" in str(too_large.value) and "MiB" in str(too_large.value)
    assert "power" not in cubes.pixel_periodograms(g, max_output_mb=0.05, return_power=False)
    # all but 3 times of cutout 1 NaN: status 2, all NaN, n_used 0; its neighbours keep their bits
    t = np.array(time)
    t[1] = np.nan
    t[1, [5, 60, 100]] = time[1, [5, 60, 100]]
    got = DevicePixelCubeBatch.from_arrays(t, flux, err).pixel_periodograms(g)
    assert got["status"].tolist() == [0, 2, 0] and not got["n_used"][1].any() and got["t_ref"][1] == time[1, 5]
    assert np.isnan(got["power"][1]).all() and np.isnan(got["peak_power"][1]).all() and np.isnan(got["peak_frequency"][1]).all()
    assert (got["peak_index"][1] == -1).all()
    for key in KEYS:
        if key != "frequency":
            assert np.array_equal(got[key][[0, 2]], whole[key][[0, 2]], equal_nan=True), key
    host = batch.pixel_periodograms_batch([PixelCube(time[b], flux[b], err[b]) for b in range(C.B)], g)
    for key in KEYS:
        assert np.array_equal(host[key], whole[key], equal_nan=True), key


def test_the_c_entry_point_refuses_bad_arguments():
    """LK_EINVAL before anything is enqueued: a NULL non-nullable buffer, counts < 1, B > 65535, N * npix or F * npix >= 2^31, a
    frequency that is not finite and > 0, another normalisation.  The valid call with the same buffers returns LK_OK."""
    import ctypes
    from lightkurve_amd import _capi
    shape, N = (3, 3), 20
    cubes = cubes_of(shape, N)
    h, npix, g = cubes.handle, shape[0] * shape[1], np.ascontiguousarray(C.grid(N))
    t_ref = np.ascontiguousarray(C.case(shape, N)[0][:, 0])
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
    out = {k: DeviceBuffer(h, n) for k, n in (("power", C.B * len(g) * npix * 8), ("peak", C.B * npix * 8), ("idx", C.B * npix * 4),
                                              ("used", C.B * npix * 4), ("status", C.B * 4))}

    def call(B=C.B, N=N, npix=npix, time=cubes.d_time.ptr, flux=cubes.d_flux.ptr, freq=g, F=len(g), norm=2, osf=1.0, t_ref=t_ref,
             power=out["power"].ptr, peak=out["peak"].ptr, idx=out["idx"].ptr, used=out["used"].ptr, status=out["status"].ptr):
        return _capi._lib.lk_cube_pixel_ls_batch_dev(
            h._h, B, N, npix, vp(time), vp(flux), None if freq is None else freq.ctypes.data_as(dp), F, norm, osf,
            None if t_ref is None else t_ref.ctypes.data_as(dp), vp(power), vp(peak), vp(idx), vp(used), vp(status),
            vp(cubes.stream or None))

    assert call() == _capi.LK_OK and call(power=None) == _capi.LK_OK
    cubes.synchronize()
    bad = [dict(time=None), dict(flux=None), dict(freq=None), dict(t_ref=None), dict(peak=None), dict(idx=None), dict(used=None),
           dict(status=None), dict(B=0), dict(N=0), dict(npix=0), dict(F=0), dict(B=65536), dict(N=2 ** 20, npix=2 ** 11),
           dict(F=2 ** 20, npix=2 ** 11), dict(norm=0), dict(norm=1), dict(norm=4), dict(osf=0.0), dict(osf=float("nan"))]
    for entry in (0.0, -1.0, np.nan, np.inf):
        f = g.copy()
        f[2] = entry
        bad.append(dict(freq=f))
    for kw in bad:
        assert call(**kw) == _capi.LK_EINVAL, kw
    cubes.synchronize()
