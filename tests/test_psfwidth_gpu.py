"""GPU: DevicePixelCubeBatch.psf_width (csrc/psfwidth.hip: cube_psfwidth_eval_kernel<S> and cube_psfwidth_step_kernel, enqueued
max_iter + 1 times) against the numpy mirror PixelCube.psf_width on the scenes of tests/psfwidth_cases.py, rendered with true
widths of 0.8 .. 1.3 px per cutout and axis and started 7 .. 15 % off.

``C.TILE`` = 16: the evaluate kernel takes a tile of 16 cadences, four lanes each, and writes one record per tile;
``C.N_VALUES`` sits on both sides of one and of two tiles.  ``C.STEP_LANES`` = 64: the step kernel adds a cutout's tile records
lane-strided over 64 lanes, so ``C.N_LONG`` has 63 tiles + 1 cadence, 64 tiles and 64 tiles + 1 cadence.  The LDS count is
psf_fit's (``C.lds_bytes``): ``C.LDS_CASES`` has (19, 19) with one star below ``C.LDS_ATTR_BYTES`` = 64 KB and with two above
it, and (33, 33) with one star just under ``C.LDS_MAX_BYTES`` = 160 KiB; ``C.TOO_LARGE`` is refused with ValueError before
anything is launched.  ``C.SETTINGS``: the defaults; ``tol=0, max_iter=6`` (a fixed count); ``max_iter=2`` (status 4);
``max_sigma=1.24`` (status 5 for cutout 1) and ``max_step=0.02`` (clamped steps).

Bounds: status, n_iter, n_cadences, n_pixels, cadence_status, NaN patterns, shapes and dtypes exact — test_psfwidth_cpu.py shows
on every compared case that no step lies within 0.1 % of tol or of max_step, no visited width within 0.1 % of a bound, no pivot
ratio between 1e-14 and 1e-9, and that the iteration contracts, so no decision depends on rounding.  sigma, trace and last_step
1e-9 px absolute; sigma_err 1e-9 relative; sigma_cov 1e-9 of sigma_err_col x sigma_err_row; chi2 1e-9 of sum w y^2 over the
contributing cadences (the house rule for float64 sums in another order).  Every comparison prints its largest difference
before it asserts (measured on an MI355X: see MEASURED below)."""
import functools

import numpy as np
import pytest

import psfwidth_cases as C
from lightkurve_amd import batch
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.device import DevicePixelCubeBatch
from lightkurve_amd.devmem import DeviceBuffer, _upload

pytestmark = pytest.mark.gpu

# largest |device - mirror| over C.CASES on an MI355X
MEASURED = "sigma 3.6e-14, trace 1.3e-13, last_step 8.7e-14 px; sigma_err 1.2e-13 relative; sigma_cov 2.4e-13; chi2 9.2e-18"

SPEC = (("sigma", np.float64, 2), ("sigma_err", np.float64, 2), ("sigma_cov", np.float64, 1), ("chi2", np.float64, 1),
        ("last_step", np.float64, 1), ("trace", np.float64, None), ("n_iter", np.int32, 1), ("n_cadences", np.int32, 1),
        ("n_pixels", np.int64, 1), ("cadence_status", np.int8, None), ("status", np.int32, 1))


def shapes(B, N, max_iter):
    return dict(sigma=(B, 2), sigma_err=(B, 2), trace=(B, max_iter + 1, 2), cadence_status=(B, N))


def run(sc, setting="default", masked=True, use_flux_err=True, cutouts=None, to_host=True, device_inputs=False, sigma0=None, **kwargs):
    """psf_width of the scene's cutouts (or of ``cutouts``, a list of their numbers) -> dict of host arrays."""
    sel = list(range(sc["B"])) if cutouts is None else list(cutouts)
    B, N = len(sel), sc["time"].shape[1]
    dev = DevicePixelCubeBatch.from_arrays(sc["time"][sel], sc["flux"][sel], sc["err"][sel])
    shifts = None if sc["shifts"] is None else tuple(np.ascontiguousarray(a[sel]) for a in sc["shifts"])
    cmask = np.ascontiguousarray(sc["cadence_mask"][sel]) if masked else None
    if device_inputs:
        shifts = None if shifts is None else tuple(_upload(dev.handle, a, dev.stream, np.float64)[0] for a in shifts)
        cmask = None if cmask is None else _upload(dev.handle, cmask.astype(np.uint8), dev.stream, np.uint8)[0]
        dev.synchronize()
    p = dict(C.SETTINGS[setting], **kwargs)
    out = dev.psf_width(sc["star_col"][sel], sc["star_row"][sel], sc["sigma0"][sel] if sigma0 is None else sigma0, shifts=shifts,
                        cadence_mask=cmask, aperture_mask=sc["mask"][sel] if masked else "all", column=C.COLUMN, row=C.ROW,
                        use_flux_err=use_flux_err, to_host=to_host, **p)
    return collect(out, dev, B, N, p.get("max_iter", C.DEFAULTS["max_iter"]))


def collect(out, dev, B, N, max_iter):
    want, got = shapes(B, N, max_iter), {}
    assert sorted(out) == sorted(k for k, _, _ in SPEC)
    for key, dt, _ in SPEC:
        a, shape = out[key], want.get(key, (B,))
        if isinstance(a, DeviceBuffer):
            a = a.download(dt, int(np.prod(shape)), stream=dev.stream).reshape(shape)
        assert a.dtype == dt and a.shape == shape, (key, a.dtype, a.shape)
        got[key] = a
    return got


@functools.lru_cache(maxsize=None)
def device_result(case):
    shape, S, N, setting, shifted, masked, use_err = case
    return run(C.scene(shape, S, N, shifted), setting, masked, use_err)


def bits(r, b=None):
    return b"".join(np.ascontiguousarray(r[k] if b is None else r[k][b]).tobytes() for k, _, _ in SPEC)


def weighted_power(sc, b, ref, masked, use_flux_err):
    """sum w y^2 over the contributing cadences of cutout b: the scale of the terms that cancel in chi2."""
    N = sc["time"].shape[1]
    y, e = sc["flux"][b].reshape(N, -1).astype(np.float64), sc["err"][b].reshape(N, -1).astype(np.float64)
    used = (sc["mask"][b].reshape(-1) if masked else np.ones(y.shape[1], dtype=bool))[None, :] & np.isfinite(y)
    if use_flux_err:
        used &= np.isfinite(e) & (e > 0)
    with np.errstate(all="ignore"):
        return np.sum(np.where(used, y * y / (e * e if use_flux_err else 1.0), 0.0), axis=1)[ref["cadence_status"] == 0].sum()


def check_against_mirror(got, sc, refs, what, use_flux_err=True, masked=True):
    worst = dict(sigma=0.0, trace=0.0, last_step=0.0, sigma_err=0.0, sigma_cov=0.0, chi2=0.0)
    for b, ref in enumerate(refs):
        for key in ("status", "n_iter", "n_cadences", "n_pixels"):
            assert got[key][b] == ref[key], (what, b, key, got[key][b], ref[key])
        assert np.array_equal(got["cadence_status"][b], ref["cadence_status"]), (what, b)
        for key in ("sigma", "sigma_err", "sigma_cov", "chi2", "last_step", "trace"):
            assert np.array_equal(np.isnan(got[key][b]), np.isnan(ref[key])), (what, b, key, got[key][b], ref[key])
        assert np.isnan(got["sigma"][b]).all() == (ref["status"] != 0)
        rows = np.isfinite(ref["trace"][:, 0])
        d = dict(trace=np.max(np.abs(got["trace"][b][rows] - ref["trace"][rows])),
                 last_step=abs(got["last_step"][b] - ref["last_step"]) if np.isfinite(ref["last_step"]) else 0.0)
        if ref["status"] == 0:
            d.update(sigma=np.max(np.abs(got["sigma"][b] - ref["sigma"])), sigma_err=np.max(np.abs(got["sigma_err"][b] / ref["sigma_err"] - 1.0)),
                     sigma_cov=abs(got["sigma_cov"][b] - ref["sigma_cov"]) / np.prod(ref["sigma_err"]),
                     chi2=abs(got["chi2"][b] - ref["chi2"]) / weighted_power(sc, b, ref, masked, use_flux_err))
        for key in d:
            worst[key] = max(worst[key], d[key])
    print("%s: max |device - mirror|: sigma %.3g, trace %.3g, last_step %.3g px; sigma_err %.3g relative; sigma_cov %.3g of the "
          "errors' product; chi2 %.3g of sum w y^2" % (what, worst["sigma"], worst["trace"], worst["last_step"], worst["sigma_err"],
                                                      worst["sigma_cov"], worst["chi2"]))
    assert max(worst.values()) < 1e-9, (what, worst)
    return worst


IDS = lambda c: "%dx%d-S%d-N%d-%s%s%s%s" % (c[0] + c[1:4] + ("" if c[4] else "-unshifted", "-masks" if c[5] else "", "" if c[6] else "-unweighted"))


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_against_mirror(case):
    shape, S, N, setting, shifted, masked, use_err = case
    check_against_mirror(device_result(case), C.scene(shape, S, N, shifted), C.mirror(*case), str(case), use_err, masked)


def test_the_lds_cases_sit_where_they_are_meant_to():
    (under, over, top), (big, big_s) = C.LDS_CASES, C.TOO_LARGE
    assert C.lds_bytes(under[0], under[1]) == 56681 < C.LDS_ATTR_BYTES < C.lds_bytes(over[0], over[1]) == 66409
    assert C.LDS_ATTR_BYTES < C.lds_bytes(top[0], top[1]) == 157761 <= C.LDS_MAX_BYTES < C.lds_bytes(big, big_s) == 174657
    assert all(C.lds_bytes(c[0], c[1], c[6]) < C.LDS_ATTR_BYTES for c in C.CASES if c not in (over, top))


def test_refusals_come_before_any_launch():
    """(33, 33) with two stars needs 174 657 bytes of LDS > LDS_MAX_BYTES: LK_EINVAL -> ValueError from the launcher's checks, and
    every parameter error is a ValueError too; nothing is launched, and the batch serves the next call."""
    shape, S = C.TOO_LARGE
    ny, nx = shape
    rng = np.random.default_rng(3)
    flux = (100 + rng.standard_normal((1, 2, ny, nx))).astype(np.float32)
    dev = DevicePixelCubeBatch.from_arrays(np.arange(2.0)[None], flux, np.ones_like(flux))
    with pytest.raises(ValueError, match="bytes of LDS"):
        dev.psf_width([nx / 2, nx / 2 + 3], [ny / 2, ny / 2], 1.5)
    out = dev.psf_width([nx / 2, nx / 2 + 3], [ny / 2, ny / 2], 1.5, use_flux_err=False, max_iter=1)     # 104 769 bytes: fits
    assert out["cadence_status"].shape == (1, 2) and out["trace"].shape == (1, 2, 2)

    sc = C.scene((5, 7), 2, 1)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    col, row, B = sc["star_col"], sc["star_row"], sc["B"]
    for kw in (dict(sigma0=0.0), dict(sigma0=np.nan), dict(star_col=np.full_like(col, np.nan)), dict(star_col=np.tile(col, (1, 5)), star_row=np.tile(row, (1, 5))),
               dict(shifts=(np.zeros((B, 2)),) * 2), dict(shifts=(np.zeros((B, 1)),)), dict(star_col=np.where(np.isnan(col), np.nan, np.inf)),
               dict(cadence_mask=np.ones((B, 2), dtype=bool)), dict(cadence_mask=np.ones((B, 1))), dict(max_iter=0), dict(max_iter=65),
               dict(max_iter=1.5), dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf), dict(max_step=0.0), dict(max_step=np.nan),
               dict(min_sigma=0.0), dict(min_sigma=np.nan), dict(max_sigma=np.inf), dict(min_sigma=1.01), dict(max_sigma=0.99),
               dict(sigma0=np.array([[1.0, 1.0]] * (B - 1) + [[1.0, 5.5]]))):
        args = dict(star_col=col, star_row=row, sigma0=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            dev.psf_width(**args)
    assert dev.psf_width(col, row, sc["sigma0"], shifts=sc["shifts"], column=C.COLUMN, row=C.ROW)["status"].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("N", [C.N_MAIN, C.N_LONG[2]])
def test_same_bits_alone_in_the_batch_and_elsewhere(N):
    shape, S = ((11, 11), 4) if N == C.N_MAIN else ((5, 7), 2)
    sc = C.scene(shape, S, N)
    whole = run(sc)
    assert bits(whole) == bits(run(sc)), "two runs differ"
    order = [2, 0, 3, 1]
    moved = run(sc, cutouts=order)
    for b in range(sc["B"]):
        alone = run(sc, cutouts=[b])
        assert bits(whole, b) == bits(alone, 0) == bits(moved, order.index(b)), b
    pair = run(sc, cutouts=[1, 0, 0])                               # among other cutouts, and twice in one batch
    assert bits(pair, 1) == bits(pair, 2) == bits(whole, 0) and bits(pair, 0) == bits(whole, 1)


def test_finished_cutouts_do_not_disturb_the_rest():
    """max_step = 0.02, max_sigma = 1.26, tol = 0, max_iter = 6: cutout 1 (from 1.235 towards 1.3) leaves the bounds at its
    second step and stops with status 5, cutout 0 takes all 6 steps and the final evaluation: it equals itself run alone."""
    sc = C.scene((11, 11), 4, C.N_MAIN)
    kw = dict(setting="fixed", max_step=0.02, max_sigma=1.26)
    both, alone = run(sc, cutouts=[1, 0], **kw), run(sc, cutouts=[0], **kw)
    assert both["status"].tolist() == [5, 0] and both["n_iter"].tolist() == [2, 6]
    assert np.isfinite(both["trace"][0, :2]).all() and np.isnan(both["trace"][0, 2:]).all() and np.isfinite(both["trace"][1]).all()
    assert bits(both, 1) == bits(alone, 0)
    ref = PixelCube(sc["time"][1], sc["flux"][1], sc["err"][1]).psf_width(tol=0.0, max_iter=6, max_step=0.02, max_sigma=1.26,
                                                                          **C.cutout_arguments(sc, 1, True))
    assert ref["status"] == 5 and ref["n_iter"] == 2 and np.max(np.abs(both["trace"][0, :2] - ref["trace"][:2])) < 1e-9
    assert np.array_equal(both["cadence_status"][0], ref["cadence_status"])


def test_tiles_that_the_cadence_mask_leaves_out_entirely():
    """cadence_mask selects the cadences 16 .. 47 of 65 alone: the tiles 0, 3 and 4 (the partial one) hold no selected cadence; the
    evaluate kernel writes their records as +0 without reading the cube, and the result is the mirror's."""
    shape, S, N = (5, 7), 2, C.N_MAIN
    sc = C.scene(shape, S, N)
    sel = np.zeros((sc["B"], N), dtype=bool)
    sel[:, C.TILE:3 * C.TILE] = True
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    got = dev.psf_width(sc["star_col"], sc["star_row"], sc["sigma0"], shifts=sc["shifts"], cadence_mask=sel, aperture_mask=sc["mask"],
                        column=C.COLUMN, row=C.ROW)
    refs = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_width(**dict(C.cutout_arguments(sc, b, True), cadence_mask=sel[b]))
            for b in range(sc["B"])]
    assert all((r["cadence_status"][~sel[0]] == 6).all() for r in refs) and [r["status"] for r in refs] == [0, 0, 0, 1]
    check_against_mirror(got, sc, refs, "whole tiles left out")


def test_input_forms_agree_bit_for_bit():
    shape, S, N = (11, 11), 4, C.N_MAIN
    sc = C.scene(shape, S, N)
    want = run(sc)
    assert bits(run(sc, device_inputs=True)) == bits(want)
    assert bits(run(sc, to_host=False)) == bits(want)
    assert bits(run(sc, to_host=False, device_inputs=True)) == bits(want)
    cubes = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]) for b in range(sc["B"])]
    out = batch.psf_width_batch(cubes, sc["star_col"], sc["star_row"], sc["sigma0"], shifts=sc["shifts"], cadence_mask=sc["cadence_mask"],
                                aperture_mask=sc["mask"], column=C.COLUMN, row=C.ROW)
    assert all(isinstance(out[k], np.ndarray) for k, _, _ in SPEC) and bits(out) == bits(want)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    held = dev.psf_width(sc["star_col"], sc["star_row"], sc["sigma0"], shifts=sc["shifts"], to_host=False)
    assert all(isinstance(held[k], DeviceBuffer) for k, _, _ in SPEC)


def test_the_chain_calibrates_itself():
    """psf_fit(sigma0) -> psf_width(shifts = the fitted shifts, on the device) -> psf_fit(the fitted sigma): the device chain
    equals the mirror chain within the bounds above, and on the clean cutout the second psf_fit's chi2 summed over the cadences
    that are ok in both is lower than the first's.  With a width that is 13 % off the first psf_fit converges linearly: at its
    defaults about half the cadences of the clean cutout stop at max_iter with status 4 (their last steps are near 1e-7 px), the
    width is fitted on the others, and with the fitted width every cadence converges in 4 .. 6 steps.  Measured on an MI355X:
    31 of 65 cadences ok in both fits, their summed chi2 25063.6 at sigma0 and 3554.1 at the fitted sigma."""
    shape, S, N = (11, 11), 4, C.N_MAIN
    sc = C.scene(shape, S, N)
    B = sc["B"]
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    kw = dict(aperture_mask=sc["mask"], column=C.COLUMN, row=C.ROW)
    _, fit1 = dev.psf_fit(sc["star_col"], sc["star_row"], sc["sigma0"], **kw)
    assert isinstance(fit1["shift_col"], DeviceBuffer)
    width = dev.psf_width(sc["star_col"], sc["star_row"], sc["sigma0"], shifts=(fit1["shift_col"], fit1["shift_row"]),
                          cadence_mask=sc["cadence_mask"], **kw)
    assert width["status"].tolist() == [0, 0, 0, 1]
    sigma = np.where(np.isnan(width["sigma"]), sc["sigma0"], width["sigma"])        # cutout 3 has none: its guess again
    _, fit2 = dev.psf_fit(sc["star_col"], sc["star_row"], sigma, to_host=True, **kw)
    chi1 = fit1["chi2"].download(np.float64, B * N, stream=dev.stream).reshape(B, N)
    st1 = fit1["cadence_status"].download(np.int8, B * N, stream=dev.stream).reshape(B, N)

    refs, mirror_sigma = [], sigma.copy()
    for b in range(B):
        cube = PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b])
        a = dict(star_col=sc["star_col"][b], star_row=sc["star_row"][b], aperture_mask=sc["mask"][b], column=C.COLUMN, row=C.ROW)
        m1 = cube.psf_fit(sigma=tuple(sc["sigma0"][b]), **a)
        mw = cube.psf_width(sigma0=tuple(sc["sigma0"][b]), shifts=(m1["shift_col"], m1["shift_row"]), cadence_mask=sc["cadence_mask"][b], **a)
        if mw["status"] == 0:
            mirror_sigma[b] = mw["sigma"]
        refs.append((mw, cube.psf_fit(sigma=tuple(mirror_sigma[b]), **a)))
    check_against_mirror(width, sc, [mw for mw, _ in refs], "the chain's psf_width")
    worst = 0.0
    for b, (_, m2) in enumerate(refs):
        assert np.array_equal(fit2["cadence_status"][b], m2["cadence_status"]), b
        ok = m2["cadence_status"] == 0
        if ok.any():
            worst = max(worst, max(np.max(np.abs(fit2[k][b][ok] - m2[k][ok])) for k in ("shift_col", "shift_row", "shift_col_err", "shift_row_err")))
    print("the chain's second psf_fit: max |device - mirror| of the shifts and their errors %.3g px" % worst)
    assert worst < 1e-9
    both = (st1[0] == 0) & (fit2["cadence_status"][0] == 0)
    first, second = chi1[0][both].sum(), fit2["chi2"][0][both].sum()
    print("clean cutout, %d cadences: summed chi2 %.1f at sigma0, %.1f at the fitted sigma" % (both.sum(), first, second))
    assert both.sum() >= N // 4 and (fit2["cadence_status"][0] == 0).all() and second < first
