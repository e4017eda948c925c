"""GPU: DevicePixelCubeBatch.psf_fit (csrc/psffit.hip: cube_psffit_kernel<S>) against the numpy mirror PixelCube.psf_fit on the
scenes of tests/psffit_cases.py, rendered with true pointing shifts of +-0.3 px per cadence.

``C.TILE`` = 16: a workgroup takes a tile of 16 cadences, four lanes each, and iterates until every cadence of the tile has
stopped; ``C.N_VALUES`` sits on both sides of one and of two tiles.  ``C.LDS_ATTR_BYTES`` = 64 KB of LDS per workgroup
(``C.lds_bytes``: psf_photometry's tile plus a factor and a derivative table per cadence): above it the launcher raises the
kernel's dynamic-LDS attribute first; ``C.LDS_CASES`` has (19, 19) with one star below it and with two above it, and (33, 33)
with one star just under ``C.LDS_MAX_BYTES`` = 160 KiB; ``C.TOO_LARGE`` is refused with ValueError before anything is launched.
``C.SETTINGS``: the defaults; ``tol=0, max_iter=8`` (a fixed count); ``max_iter=2`` (status 4 everywhere), ``max_shift=0.1``
(status 5 where the true shift exceeds it) and ``max_step=0.05`` (clamped first steps).

Bounds: statuses, n_used, n_iter, NaN patterns and shapes exact — test_psffit_cpu.py shows on every compared case that no step
lies within 0.1 % of tol, no unclamped step at max_step, no excursion at max_shift, no pivot ratio between 1e-14 and 1e-9, and
that the iteration contracts, so no decision depends on rounding and rounding differences shrink from step to step.  Shifts,
their errors and last_step 1e-9 px absolute; flux and background 1e-9 of the cutout's largest |flux|; flux_err 1e-9 relative;
chi2 1e-9 of sum w y^2 (the house rule for float64 sums in another order).  Every comparison prints its largest difference
before it asserts (measured on an MI355X: shifts and last_step 3.2e-14 px, shift errors 5.1e-15 px, flux 3.0e-14, background
2.0e-15, flux_err 3.0e-14, chi2 2.9e-16; psf_photometry at the returned shifts: flux, flux_err and background equal, chi2
2.7e-16 relative, not bit-equal)."""
import functools

import numpy as np
import pytest

import psffit_cases as C
from lightkurve_amd import batch
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.device import DeviceLightCurveBatch, DevicePixelCubeBatch
from lightkurve_amd.devmem import DeviceBuffer, _upload

pytestmark = pytest.mark.gpu

FLOATS = ("background", "chi2", "shift_col", "shift_row", "shift_col_err", "shift_row_err", "last_step")
INFO = tuple((k, np.float64) for k in FLOATS) + (("n_iter", np.int32), ("n_used", np.int32), ("cadence_status", np.int8),
                                                 ("status", np.int32), ("star_off", np.int32))


def run(sc, setting="default", start=False, masked=True, use_flux_err=True, cutouts=None, to_host=True, device_start=False):
    """psf_fit of the scene's cutouts (or of ``cutouts``, a list of their numbers) -> dict of host arrays: flux, flux_err, time
    (rows, N), the keys of INFO, and meta."""
    sel = list(range(sc["B"])) if cutouts is None else list(cutouts)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"][sel], sc["flux"][sel], sc["err"][sel])
    s0 = None
    if start:
        s0 = tuple(np.ascontiguousarray(a[sel]) for a in sc["shifts0"])
        if device_start:
            s0 = tuple(_upload(dev.handle, a, dev.stream, np.float64)[0] for a in s0)
            dev.synchronize()
    lcs, info = dev.psf_fit(sc["star_col"][sel], sc["star_row"][sel], sc["sigma"][sel], shifts0=s0,
                            aperture_mask=sc["mask"][sel] if masked else "all", column=C.COLUMN, row=C.ROW,
                            use_flux_err=use_flux_err, to_host=to_host, **C.SETTINGS[setting])
    return collect(lcs, info, len(sel), sc["time"].shape[1])


def collect(lcs, info, B, N, spec=INFO):
    assert isinstance(lcs, DeviceLightCurveBatch)
    host = lcs.to_host()
    rows = len(lcs)
    assert np.array_equal(host.n_off, np.arange(rows + 1) * N)
    out = dict(flux=host.flux.reshape(rows, N), flux_err=host.flux_err.reshape(rows, N), time=host.time.reshape(rows, N), meta=host.meta)
    for key, dt in spec:
        a = info[key]
        if isinstance(a, DeviceBuffer):
            a = a.download(dt, {"status": B, "star_off": B + 1}.get(key, B * N), stream=lcs.stream)
        assert a.dtype == dt, key
        out[key] = a.reshape(-1) if key in ("status", "star_off") else a.reshape(B, N)
    return out


@functools.lru_cache(maxsize=None)
def device_result(case):
    shape, S, N, setting, start, masked, use_err = case
    return run(C.scene(shape, S, N), setting, start, masked, use_err)


def bits(r, spec=INFO):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("flux", "flux_err", "time") + tuple(k for k, _ in spec))


def weighted_power(sc, b, masked, use_flux_err):
    """sum w y^2 per cadence of cutout b: the scale of the terms that cancel in chi2."""
    N = sc["time"].shape[1]
    y, e = sc["flux"][b].reshape(N, -1).astype(np.float64), sc["err"][b].reshape(N, -1).astype(np.float64)
    used = (sc["mask"][b].reshape(-1) if masked else np.ones(y.shape[1], dtype=bool))[None, :] & np.isfinite(y)
    if use_flux_err:
        used &= np.isfinite(e) & (e > 0)
    with np.errstate(all="ignore"):
        return np.sum(np.where(used, y * y / (e * e if use_flux_err else 1.0), 0.0), axis=1)


def check_against_mirror(got, sc, refs, what, use_flux_err=True, masked=True):
    B, N = sc["B"], sc["time"].shape[1]
    counts = [len(r["star_index"]) for r in refs]
    assert got["star_off"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert got["flux"].shape == got["flux_err"].shape == got["time"].shape == (sum(counts), N)
    assert got["status"].tolist() == [r["status"] for r in refs], what
    worst = dict(flux=0.0, background=0.0, flux_err=0.0, chi2=0.0, shift=0.0, shift_err=0.0, last_step=0.0)
    for b, ref in enumerate(refs):
        r0, r1 = got["star_off"][b], got["star_off"][b + 1]
        for key in ("cadence_status", "n_used", "n_iter"):
            assert np.array_equal(got[key][b], ref[key]), (what, b, key, got[key][b], ref[key])
        assert np.array_equal(got["time"][r0:r1], np.tile(sc["time"][b], (r1 - r0, 1)), equal_nan=True)
        ok = ref["cadence_status"] == 0
        for key, mine, theirs in ([("flux", got["flux"][r0:r1], ref["flux"]), ("flux_err", got["flux_err"][r0:r1], ref["flux_err"])]
                                  + [(k, got[k][b], ref[k]) for k in FLOATS]):
            assert np.array_equal(np.isnan(mine), np.isnan(theirs)), (what, b, key)
            if key != "last_step":
                assert np.array_equal(np.isnan(theirs), np.broadcast_to(~ok, theirs.shape)), (what, b, key)
        for row, s in zip(range(r0, r1), ref["star_index"]):
            m = got["meta"][row]
            assert m["STAR_INDEX"] == s and m["STAR_COL"] == sc["star_col"][b, s] and m["STAR_ROW"] == sc["star_row"][b, s]
        stepped = np.isfinite(ref["last_step"])
        d = dict(last_step=np.max(np.abs(got["last_step"][b][stepped] - ref["last_step"][stepped])) if stepped.any() else 0.0)
        if ok.any():
            top, wy2 = np.max(np.abs(ref["flux"][:, ok])), weighted_power(sc, b, masked, use_flux_err)
            d.update(flux=np.max(np.abs(got["flux"][r0:r1][:, ok] - ref["flux"][:, ok])) / top,
                     background=np.max(np.abs(got["background"][b][ok] - ref["background"][ok])) / top,
                     flux_err=np.max(np.abs(got["flux_err"][r0:r1][:, ok] / ref["flux_err"][:, ok] - 1.0)),
                     chi2=np.max(np.abs(got["chi2"][b][ok] - ref["chi2"][ok]) / wy2[ok]),
                     shift=max(np.max(np.abs(got[k][b][ok] - ref[k][ok])) for k in ("shift_col", "shift_row")),
                     shift_err=max(np.max(np.abs(got[k][b][ok] - ref[k][ok])) for k in ("shift_col_err", "shift_row_err")))
        for key in d:
            worst[key] = max(worst[key], d[key])
    print("%s: max |device - mirror|: shifts %.3g, their errors %.3g, last_step %.3g px; flux %.3g, background %.3g of the largest "
          "flux; flux_err %.3g relative; chi2 %.3g of sum w y^2" % (what, worst["shift"], worst["shift_err"], worst["last_step"],
                                                                    worst["flux"], worst["background"], worst["flux_err"], worst["chi2"]))
    assert max(worst.values()) < 1e-9, (what, worst)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: "%dx%d-S%d-N%d-%s%s%s%s" % (c[0] + c[1:4] + ("-start" if c[4] else "", "-masks" if c[5] else "",
                                                                                                   "" if c[6] else "-unweighted")))
def test_against_mirror(case):
    shape, S, N, setting, start, masked, use_err = case
    check_against_mirror(device_result(case), C.scene(shape, S, N), C.mirror(*case), str(case), use_err, masked)


def test_the_lds_cases_sit_where_they_are_meant_to():
    (under, over, top), (big, big_s) = C.LDS_CASES, C.TOO_LARGE
    assert C.lds_bytes(under[0], under[1]) == 56681 < C.LDS_ATTR_BYTES < C.lds_bytes(over[0], over[1]) == 66409
    assert C.LDS_ATTR_BYTES < C.lds_bytes(top[0], top[1]) == 157761 <= C.LDS_MAX_BYTES < C.lds_bytes(big, big_s) == 174657
    assert all(C.lds_bytes(c[0], c[1], c[6]) < C.LDS_ATTR_BYTES for c in C.CASES if c not in (over, top))


def test_a_cutout_beyond_the_lds_limit_is_refused():
    """(33, 33) with two stars needs 174 657 bytes of LDS > LDS_MAX_BYTES: LK_EINVAL -> ValueError from the launcher's checks,
    which come before every launch; the batch serves the next call."""
    shape, S = C.TOO_LARGE
    ny, nx = shape
    rng = np.random.default_rng(3)
    flux = (100 + rng.standard_normal((1, 2, ny, nx))).astype(np.float32)
    dev = DevicePixelCubeBatch.from_arrays(np.arange(2.0)[None], flux, np.ones_like(flux))
    with pytest.raises(ValueError, match="bytes of LDS"):
        dev.psf_fit([nx / 2, nx / 2 + 3], [ny / 2, ny / 2], 1.5)
    lcs, info = dev.psf_fit([nx / 2, nx / 2 + 3], [ny / 2, ny / 2], 1.5, use_flux_err=False, to_host=True)     # 104 769 bytes: fits
    assert info["cadence_status"].shape == (1, 2) and len(lcs) == 2


SHAPE, S, N = (11, 11), 4, C.N_MAIN


def test_same_bits_alone_in_the_batch_and_elsewhere():
    sc = C.scene(SHAPE, S, N)
    for setting, start in (("default", False), ("fixed", True)):
        whole = run(sc, setting, start)
        assert bits(whole) == bits(run(sc, setting, start)), "two runs differ"
        order = [2, 0, 3, 1]
        moved = run(sc, setting, start, cutouts=order)
        for b in range(sc["B"]):
            alone = run(sc, setting, start, cutouts=[b])
            for r, pos in ((whole, b), (moved, order.index(b))):
                r0, r1 = r["star_off"][pos], r["star_off"][pos + 1]
                for key in ("flux", "flux_err", "time"):
                    assert r[key][r0:r1].tobytes() == alone[key].tobytes(), (setting, b, key)
                for key, _ in INFO[:-1]:
                    assert r[key][pos].tobytes() == alone[key][0].tobytes(), (setting, b, key)


def test_to_host_forms_start_forms_and_the_host_batch_function():
    sc = C.scene(SHAPE, S, N)
    want = run(sc, start=True)
    assert bits(run(sc, start=True, to_host=False)) == bits(want)
    assert bits(run(sc, start=True, device_start=True)) == bits(want)
    cubes = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]) for b in range(sc["B"])]
    lcs, info = batch.psf_fit_batch(cubes, sc["star_col"], sc["star_row"], sc["sigma"], shifts0=sc["shifts0"], aperture_mask=sc["mask"],
                                    column=C.COLUMN, row=C.ROW)
    assert all(isinstance(info[k], np.ndarray) for k, _ in INFO)
    assert bits(collect(lcs, info, sc["B"], N)) == bits(want)


def test_the_fitted_shifts_feed_psf_photometry_on_the_device():
    """The returned shift buffers, handed to psf_photometry(shifts=) without a host round trip, reproduce the fit's flux,
    flux_err, background and chi2 on every ok cadence within 1e-9 (a cadence that is not ok has NaN shifts: status 1 there)."""
    sc = C.scene(SHAPE, S, N)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    kw = dict(aperture_mask=sc["mask"], column=C.COLUMN, row=C.ROW)
    lcs, info = dev.psf_fit(sc["star_col"], sc["star_row"], sc["sigma"], **kw)
    assert isinstance(info["shift_col"], DeviceBuffer) and isinstance(info["shift_row"], DeviceBuffer)
    again = dev.psf_photometry(sc["star_col"], sc["star_row"], sc["sigma"], shifts=(info["shift_col"], info["shift_row"]), **kw)
    spec = tuple(kv for kv in INFO if kv[0] in ("background", "chi2", "n_used", "cadence_status", "status", "star_off"))
    fit, phot = collect(lcs, info, sc["B"], N), collect(again[0], again[1], sc["B"], N, spec)
    ok = fit["cadence_status"] == 0
    assert ok.any() and np.array_equal(phot["cadence_status"] == 0, ok) and np.array_equal(phot["n_used"], fit["n_used"])
    rows = np.repeat(ok, np.diff(fit["star_off"]), axis=0)
    worst, same = {}, True
    for key, sel in (("flux", rows), ("flux_err", rows), ("background", ok), ("chi2", ok)):
        a, m = phot[key][sel], fit[key][sel]
        worst[key] = np.max(np.abs(a - m) / np.abs(m))
        same = same and a.tobytes() == m.tobytes()
    print("psf_photometry at the fitted shifts against psf_fit, relative: %s; bit-equal: %s" % (worst, same))
    assert max(worst.values()) < 1e-9, worst


def test_arguments_are_checked():
    sc = C.scene((5, 7), 2, 1)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    col, row = sc["star_col"], sc["star_row"]
    for kw in (dict(sigma=0.0), dict(sigma=np.nan), dict(star_col=np.full_like(col, np.nan)), dict(star_col=np.tile(col, (1, 5)), star_row=np.tile(row, (1, 5))),
               dict(shifts0=(np.zeros((sc["B"], 2)),) * 2), dict(shifts0=(np.zeros((sc["B"], 1)),)), dict(star_col=np.where(np.isnan(col), np.nan, np.inf)),
               dict(max_iter=0), dict(max_iter=65), dict(max_iter=1.5), dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf), dict(max_step=0.0),
               dict(max_step=np.nan), dict(max_shift=0.0), dict(max_shift=-2.0)):
        args = dict(star_col=col, star_row=row, sigma=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            dev.psf_fit(**args)


def test_chain_finds_the_transit_and_the_shift_fit_removes_the_motion():
    """Two blended stars 1.7 px apart that share a random walk of the pointing within +-0.3 px; star 1 carries a box transit:
    psf_fit -> remove_nans -> normalize -> bls puts star 1's peak at the injected period, and the normalised scatter of star 0
    (constant) from psf_fit is smaller than from psf_photometry without shifts on the same cube, which turns the motion into
    flux."""
    shape, N, period, depth, dur = (11, 11), 1500, 2.5, 0.02, 0.15
    rng = np.random.default_rng(11)
    time = 2000.0 + np.arange(N) * 0.01
    col, row, sig = np.array([4.2, 5.9]), np.array([5.1, 5.3]), 1.1
    walk = np.cumsum(rng.normal(0.0, 0.02, (2, N)), axis=1)
    walk = 0.3 * walk / np.max(np.abs(walk), axis=1, keepdims=True)
    in_transit = np.abs((time - 2000.7 + period / 2) % period - period / 2) < dur / 2
    f = np.stack([np.full(N, 6000.0), 4000.0 * np.where(in_transit, 1 - depth, 1.0)])
    img = np.full((N,) + shape, 30.0)
    for n in range(N):
        for s in range(2):
            img[n] += f[s, n] * C.psf_image(shape, col[s] + walk[0, n], row[s] + walk[1, n], sig, sig)
    err = np.sqrt(img / 25.0)
    flux = (img + err * rng.standard_normal(img.shape)).astype(np.float32)
    flux[700] = np.nan                                                      # one failed cadence: remove_nans drops it
    dev = DevicePixelCubeBatch.from_arrays(time[None], flux[None], err.astype(np.float32)[None])
    lcs, info = dev.psf_fit(col, row, sig, to_host=True)
    assert info["cadence_status"][0, 700] == 2 and (info["cadence_status"] == 0).sum() == N - 1
    moved = np.delete(np.abs(np.stack([info["shift_col"][0], info["shift_row"][0]]) - walk), 700, axis=1)
    print("largest |fitted - true shift| %.4f px" % moved.max())
    assert moved.max() < 0.05
    clean = lcs.remove_nans().normalize()
    assert np.diff(clean.n_off).tolist() == [N - 1, N - 1]
    pk = clean.bls(np.linspace(1.5, 3.5, 401), duration=[dur]).peaks()
    print("BLS peaks: period %s, depth %s" % (pk["period"], pk["depth"]))
    assert abs(pk["period"][1] - period) <= 0.005 + 1e-12 and 0.5 * depth < pk["depth"][1] < 1.5 * depth
    fixed = dev.psf_photometry(col, row, sig)[0].remove_nans().normalize()
    scatter = [np.std(lc.to_host().flux.reshape(2, N - 1)[0]) for lc in (clean, fixed)]
    print("normalised scatter of the constant star: psf_fit %.5f, psf_photometry without shifts %.5f" % tuple(scatter))
    assert scatter[0] < scatter[1]
