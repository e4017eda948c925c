"""GPU: DevicePixelCubeBatch.psf_positions (csrc/psfpos.hip: cube_psfpos_eval_kernel<S> and cube_psfpos_step_kernel, enqueued
max_iter + 1 times) against the numpy mirror PixelCube.psf_positions on the scenes of tests/psfpos_cases.py, rendered at the true
positions and started 0.1 .. 0.3 px off per star and axis.

``C.TILE`` = 16: the evaluate kernel takes a tile of 16 cadences, four lanes each, and writes one record per tile;
``C.N_VALUES`` sits on both sides of one and of two tiles.  ``C.STEP_LANES`` = 64: the step kernel adds a cutout's tile records
lane-strided over 64 lanes, so ``C.N_LONG`` has 63 tiles + 1 cadence, 64 tiles and 64 tiles + 1 cadence.  The LDS count is
psf_fit's plus the parked L^-1 C (``C.lds_bytes``): ``C.LDS_CASES`` has (19, 19) with one star below ``C.LDS_ATTR_BYTES`` = 64
KB and with two above it (as (11, 11) with 8 stars now is), and (33, 33) with one star just under ``C.LDS_MAX_BYTES`` = 160
KiB; ``C.TOO_LARGE`` is refused with ValueError before anything is launched.  ``C.SETTINGS``: the defaults; ``tol=0, max_iter=6`` (a fixed count); ``max_iter=2``
(status 4); ``max_offset=0.24`` (status 5 for cutout 1) and ``max_step=0.02`` (clamped steps).  ``subset`` cases fit the stars
of the even slots alone.

Bounds: status, n_iter, n_cadences, n_pixels, cadence_status, NaN patterns, shapes and dtypes exact — test_psfpos_cpu.py shows on
every compared case that no step lies within 0.1 % of tol or of max_step, no visited offset within 0.1 % of max_offset, no pivot
ratio between 1e-14 and 1e-9, and that the iteration contracts, so no decision depends on rounding.  star_col, star_row, trace
and last_step 1e-9 px absolute; the errors 1e-9 relative; position_cov 1e-9 of the product of the two errors; chi2 1e-9 of sum
w y^2 over the contributing cadences (the house rule for float64 sums in another order).  Every comparison prints its largest
difference before it asserts (measured on an MI355X: see MEASURED below)."""
import functools

import numpy as np
import pytest

import psfpos_cases as C
from lightkurve_amd import batch
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.device import DevicePixelCubeBatch
from lightkurve_amd.devmem import DeviceBuffer, _upload

pytestmark = pytest.mark.gpu

# largest |device - mirror| over C.CASES on an MI355X
MEASURED = ("positions 1.4e-14, trace 1.4e-14, last_step 6.6e-16 px; errors 5.3e-15 relative; position_cov 1.1e-14; chi2 8.5e-18 "
            "(the positions are near 100 and 200 px: one unit in their last place is 1.4e-14 or 2.8e-14 px)")

SPEC = (("star_col", np.float64), ("star_row", np.float64), ("star_col_err", np.float64), ("star_row_err", np.float64),
        ("position_cov", np.float64), ("chi2", np.float64), ("last_step", np.float64), ("trace", np.float64), ("n_iter", np.int32),
        ("n_cadences", np.int32), ("n_pixels", np.int64), ("cadence_status", np.int8), ("status", np.int32))


def shapes(B, N, S, max_iter):
    return dict(star_col=(B, S), star_row=(B, S), star_col_err=(B, S), star_row_err=(B, S), position_cov=(B, 2 * S, 2 * S),
                trace=(B, max_iter + 1, 2 * S), cadence_status=(B, N))


def run(sc, setting="default", masked=True, use_flux_err=True, subset=False, cutouts=None, to_host=True, device_inputs=False, **kwargs):
    """psf_positions of the scene's cutouts (or of ``cutouts``, a list of their numbers) -> dict of host arrays."""
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
    col, row, fit = C.start(sc, subset)
    out = dev.psf_positions(col[sel], row[sel], sc["sigma"][sel], shifts=shifts, cadence_mask=cmask, fit_star=None if fit is None else fit[sel],
                            aperture_mask=sc["mask"][sel] if masked else "all", column=C.COLUMN, row=C.ROW, use_flux_err=use_flux_err,
                            to_host=to_host, **p)
    return collect(out, dev, B, N, col.shape[1], p.get("max_iter", C.DEFAULTS["max_iter"]))


def collect(out, dev, B, N, S, max_iter):
    want, got = shapes(B, N, S, max_iter), {}
    assert sorted(out) == sorted(k for k, _ in SPEC)
    for key, dt in SPEC:
        a, shape = out[key], want.get(key, (B,))
        if isinstance(a, DeviceBuffer):
            a = a.download(dt, int(np.prod(shape)), stream=dev.stream).reshape(shape)
        assert a.dtype == dt and a.shape == shape, (key, a.dtype, a.shape)
        got[key] = a
    return got


@functools.lru_cache(maxsize=None)
def device_result(case):
    shape, S, N, setting, shifted, masked, use_err, subset = case
    return run(C.scene(shape, S, N, shifted), setting, masked, use_err, subset)


def bits(r, b=None):
    return b"".join(np.ascontiguousarray(r[k] if b is None else r[k][b]).tobytes() for k, _ in SPEC)


def weighted_power(sc, b, ref, masked, use_flux_err):
    """sum w y^2 over the contributing cadences of cutout b: the scale of the terms that cancel in chi2."""
    N = sc["time"].shape[1]
    y, e = sc["flux"][b].reshape(N, -1).astype(np.float64), sc["err"][b].reshape(N, -1).astype(np.float64)
    used = (sc["mask"][b].reshape(-1) if masked else np.ones(y.shape[1], dtype=bool))[None, :] & np.isfinite(y)
    if use_flux_err:
        used &= np.isfinite(e) & (e > 0)
    with np.errstate(all="ignore"):
        return np.sum(np.where(used, y * y / (e * e if use_flux_err else 1.0), 0.0), axis=1)[ref["cadence_status"] == 0].sum()


FLOATS = ("star_col", "star_row", "star_col_err", "star_row_err", "position_cov", "chi2", "last_step", "trace")


def check_against_mirror(got, sc, refs, what, use_flux_err=True, masked=True):
    worst = dict(position=0.0, trace=0.0, last_step=0.0, err=0.0, cov=0.0, chi2=0.0)
    for b, ref in enumerate(refs):
        for key in ("status", "n_iter", "n_cadences", "n_pixels"):
            assert got[key][b] == ref[key], (what, b, key, got[key][b], ref[key])
        assert np.array_equal(got["cadence_status"][b], ref["cadence_status"]), (what, b)
        for key in FLOATS:
            assert np.array_equal(np.isnan(got[key][b]), np.isnan(ref[key])), (what, b, key, got[key][b], ref[key])
        fitted = np.zeros(len(ref["star_col"]), dtype=bool)
        fitted[ref["fitted_index"]] = True
        assert np.isnan(got["star_col"][b][fitted]).all() == (ref["status"] != 0)
        for key in ("star_col", "star_row"):                   # a star that is not fitted: its input bits
            assert got[key][b][~fitted].tobytes() == ref[key][~fitted].tobytes(), (what, b, key)
        rows = np.isfinite(ref["trace"]).any(axis=1)
        d = dict(trace=np.nanmax(np.abs(got["trace"][b][rows] - ref["trace"][rows])),
                 last_step=abs(got["last_step"][b] - ref["last_step"]) if np.isfinite(ref["last_step"]) else 0.0)
        if ref["status"] == 0:
            err = np.concatenate([ref["star_col_err"][fitted], ref["star_row_err"][fitted]])
            gerr = np.concatenate([got["star_col_err"][b][fitted], got["star_row_err"][b][fitted]])
            full = np.stack([ref["star_col_err"], ref["star_row_err"]], axis=1).reshape(-1)       # index 2 slot + axis
            with np.errstate(invalid="ignore"):
                cov = np.abs(got["position_cov"][b] - ref["position_cov"]) / (full[:, None] * full[None, :])
            d.update(position=max(np.max(np.abs(got[k][b] - ref[k])[fitted]) for k in ("star_col", "star_row")),
                     err=np.max(np.abs(gerr / err - 1.0)), cov=np.nanmax(cov),
                     chi2=abs(got["chi2"][b] - ref["chi2"]) / weighted_power(sc, b, ref, masked, use_flux_err))
        for key in d:
            worst[key] = max(worst[key], d[key])
    print("%s: max |device - mirror|: positions %.3g, trace %.3g, last_step %.3g px; errors %.3g relative; position_cov %.3g of the "
          "errors' product; chi2 %.3g of sum w y^2" % (what, worst["position"], worst["trace"], worst["last_step"], worst["err"],
                                                      worst["cov"], worst["chi2"]))
    assert max(worst.values()) < 1e-9, (what, worst)
    return worst


IDS = lambda c: "%dx%d-S%d-N%d-%s%s%s%s%s" % (c[0] + c[1:4] + ("" if c[4] else "-unshifted", "-masks" if c[5] else "",
                                                               "" if c[6] else "-unweighted", "-subset" if c[7] else ""))


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_against_mirror(case):
    shape, S, N, setting, shifted, masked, use_err, subset = case
    check_against_mirror(device_result(case), C.scene(shape, S, N, shifted), C.mirror(*case), str(case), use_err, masked)


def test_the_lds_cases_sit_where_they_are_meant_to():
    (under, over, top), (big, big_s) = C.LDS_CASES, C.TOO_LARGE
    assert C.lds_bytes(under[0], under[1]) == 57193 < C.LDS_ATTR_BYTES < C.lds_bytes(over[0], over[1]) == 67945
    assert C.LDS_ATTR_BYTES < C.lds_bytes(top[0], top[1]) == 158273 <= C.LDS_MAX_BYTES < C.lds_bytes(big, big_s) == 176193
    # the parked L^-1 C lifts (11, 11) with 8 stars above LDS_ATTR_BYTES as well (79 481 bytes, 61 049 in psf_fit's count)
    above = [c for c in C.CASES if C.lds_bytes(c[0], c[1], c[6]) > C.LDS_ATTR_BYTES]
    assert set(above) == {over, top} | {c for c in C.CASES if c[:2] == ((11, 11), 8)} and len(above) == 4
    assert C.lds_bytes((11, 11), 8) == 79481


def test_refusals_come_before_any_launch():
    """(33, 33) with two stars needs 176 193 bytes of LDS > LDS_MAX_BYTES: LK_EINVAL -> ValueError from the launcher's checks, and
    every parameter error is a ValueError too; nothing is launched, and the batch serves the next call."""
    shape, S = C.TOO_LARGE
    ny, nx = shape
    rng = np.random.default_rng(3)
    flux = (100 + rng.standard_normal((1, 2, ny, nx))).astype(np.float32)
    dev = DevicePixelCubeBatch.from_arrays(np.arange(2.0)[None], flux, np.ones_like(flux))
    with pytest.raises(ValueError, match="bytes of LDS"):
        dev.psf_positions([nx / 2, nx / 2 + 3], [ny / 2, ny / 2], 1.5)
    out = dev.psf_positions([nx / 2, nx / 2 + 3], [ny / 2, ny / 2], 1.5, use_flux_err=False, max_iter=1)     # 106 305 bytes: fits
    assert out["cadence_status"].shape == (1, 2) and out["trace"].shape == (1, 2, 4)

    sc = C.scene((5, 7), 2, 1)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    col, row, B = sc["star_col"], sc["star_row"], sc["B"]
    none_fitted = np.ones((B, 2), dtype=bool)
    none_fitted[2] = [True, False]                              # cutout 2 has its one star in slot 1
    for kw in (dict(sigma=0.0), dict(sigma=np.nan), dict(star_col=np.full_like(col, np.nan)), dict(star_col=np.tile(col, (1, 5)), star_row=np.tile(row, (1, 5))),
               dict(shifts=(np.zeros((B, 2)),) * 2), dict(shifts=(np.zeros((B, 1)),)), dict(star_col=np.where(np.isnan(col), np.nan, np.inf)),
               dict(cadence_mask=np.ones((B, 2), dtype=bool)), dict(cadence_mask=np.ones((B, 1))), dict(max_iter=0), dict(max_iter=65),
               dict(max_iter=1.5), dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf), dict(max_step=0.0), dict(max_step=np.nan),
               dict(max_offset=0.0), dict(max_offset=-1.0), dict(max_offset=np.nan), dict(fit_star=np.zeros(2, dtype=bool)),
               dict(fit_star=np.ones((B, 3), dtype=bool)), dict(fit_star=np.ones((B, 2))), dict(fit_star=none_fitted)):
        args = dict(star_col=col, star_row=row, sigma=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            dev.psf_positions(**args)
    assert dev.psf_positions(col, row, sc["sigma"], shifts=sc["shifts"], column=C.COLUMN, row=C.ROW)["status"].tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("N", [C.N_MAIN, C.N_LONG[2]])
def test_same_bits_alone_in_the_batch_and_elsewhere(N):
    """A cutout alone, at another batch position, twice in one batch and in two runs; and next to a cutout that stopped early:
    with tol = 0, max_iter = 6, max_step = 0.2 and max_offset = 0.24 cutout 1 (0.27 .. 0.3 px from the truth) takes a clamped
    step, leaves max_offset at its second and stops with status 5, while cutout 0 takes all 6 steps and the final evaluation."""
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

    kw = dict(setting="fixed", max_step=0.2, max_offset=0.24)
    both, alone = run(sc, cutouts=[1, 0], **kw), run(sc, cutouts=[0], **kw)
    assert both["status"].tolist() == [5, 0] and both["n_iter"].tolist() == [2, 6]
    assert np.isfinite(both["trace"][0, :2]).all() and np.isnan(both["trace"][0, 2:]).all() and np.isfinite(both["trace"][1]).all()
    assert bits(both, 1) == bits(alone, 0)
    ref = PixelCube(sc["time"][1], sc["flux"][1], sc["err"][1]).psf_positions(tol=0.0, max_iter=6, max_step=0.2, max_offset=0.24,
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
    got = dev.psf_positions(sc["star_col"], sc["star_row"], sc["sigma"], shifts=sc["shifts"], cadence_mask=sel, aperture_mask=sc["mask"],
                            column=C.COLUMN, row=C.ROW)
    refs = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_positions(**dict(C.cutout_arguments(sc, b, True), cadence_mask=sel[b]))
            for b in range(sc["B"])]
    assert all((r["cadence_status"][~sel[0]] == 6).all() for r in refs) and [r["status"] for r in refs] == [0, 0, 0, 1]
    check_against_mirror(got, sc, refs, "whole tiles left out")


def test_input_forms_agree_bit_for_bit():
    shape, S, N = (11, 11), 4, C.N_MAIN
    sc = C.scene(shape, S, N)
    for subset in (False, True):
        want = run(sc, subset=subset)
        assert bits(run(sc, subset=subset, device_inputs=True)) == bits(want)
        assert bits(run(sc, subset=subset, to_host=False)) == bits(want)
        assert bits(run(sc, subset=subset, to_host=False, device_inputs=True)) == bits(want)
        col, row, fit = C.start(sc, subset)
        cubes = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]) for b in range(sc["B"])]
        out = batch.psf_positions_batch(cubes, col, row, sc["sigma"], shifts=sc["shifts"], cadence_mask=sc["cadence_mask"], fit_star=fit,
                                        aperture_mask=sc["mask"], column=C.COLUMN, row=C.ROW)
        assert all(isinstance(out[k], np.ndarray) for k, _ in SPEC) and bits(out) == bits(want)
        if subset:                                                  # a star that is not fitted returns its input bits
            assert want["star_col"][~fit].tobytes() == col[~fit].tobytes() and want["star_row"][~fit].tobytes() == row[~fit].tobytes()
            one = run(sc, subset=True, cutouts=[0])
            shared = DevicePixelCubeBatch.from_arrays(sc["time"][:1], sc["flux"][:1], sc["err"][:1]).psf_positions(
                col[0], row[0], sc["sigma"][:1], shifts=tuple(a[:1] for a in sc["shifts"]), cadence_mask=sc["cadence_mask"][:1],
                fit_star=fit[0], aperture_mask=sc["mask"][:1], column=C.COLUMN, row=C.ROW)           # the (S_max,) forms
            assert bits(shared) == bits(one)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    held = dev.psf_positions(sc["star_col"], sc["star_row"], sc["sigma"], shifts=sc["shifts"], to_host=False)
    assert all(isinstance(held[k], DeviceBuffer) for k, _ in SPEC)


def test_the_chain_calibrates_itself():
    """psf_fit at the offset positions -> psf_positions(shifts = the fitted shifts, on the device) -> psf_fit at the fitted
    positions: the device chain equals the mirror chain within the bounds above, and on the clean cutout the second psf_fit's
    chi2 summed over the cadences that are ok in both is lower than the first's.  Both psf_fit calls take a fixed count of steps
    (tol = 0, max_iter = 8), so that no cadence's status hangs on a step that lies near tol while the positions are still wrong.
    The shifts of the first fit absorb the stars' mean offset (the fit is conditional on them: a common translation is theirs),
    psf_positions then fits what differs from star to star.  Measured on an MI355X: all 65 cadences of the clean cutout ok in both
    fits, their summed chi2 47841.1 at the given positions and 7313.7 at the fitted ones."""
    shape, S, N = (11, 11), 4, C.N_MAIN
    sc = C.scene(shape, S, N)
    B = sc["B"]
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    kw = dict(aperture_mask=sc["mask"], column=C.COLUMN, row=C.ROW)
    fixed = dict(tol=0.0, max_iter=8)
    _, fit1 = dev.psf_fit(sc["star_col"], sc["star_row"], sc["sigma"], **fixed, **kw)
    assert isinstance(fit1["shift_col"], DeviceBuffer)
    pos = dev.psf_positions(sc["star_col"], sc["star_row"], sc["sigma"], shifts=(fit1["shift_col"], fit1["shift_row"]),
                            cadence_mask=sc["cadence_mask"], **kw)
    assert pos["status"].tolist() == [0, 0, 0, 1]
    ok = (pos["status"] == 0)[:, None]
    col2, row2 = np.where(ok, pos["star_col"], sc["star_col"]), np.where(ok, pos["star_row"], sc["star_row"])     # cutout 3: as given
    _, fit2 = dev.psf_fit(col2, row2, sc["sigma"], to_host=True, **fixed, **kw)
    chi1 = fit1["chi2"].download(np.float64, B * N, stream=dev.stream).reshape(B, N)
    st1 = fit1["cadence_status"].download(np.int8, B * N, stream=dev.stream).reshape(B, N)

    refs = []
    for b in range(B):
        cube = PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b])
        a = dict(sigma=tuple(sc["sigma"][b]), aperture_mask=sc["mask"][b], column=C.COLUMN, row=C.ROW)
        m1 = cube.psf_fit(star_col=sc["star_col"][b], star_row=sc["star_row"][b], **fixed, **a)
        mp = cube.psf_positions(star_col=sc["star_col"][b], star_row=sc["star_row"][b], shifts=(m1["shift_col"], m1["shift_row"]),
                                cadence_mask=sc["cadence_mask"][b], **a)
        mc, mr = (mp["star_col"], mp["star_row"]) if mp["status"] == 0 else (sc["star_col"][b], sc["star_row"][b])
        refs.append((mp, cube.psf_fit(star_col=mc, star_row=mr, **fixed, **a)))
    check_against_mirror(pos, sc, [mp for mp, _ in refs], "the chain's psf_positions")
    worst = 0.0
    for b, (_, m2) in enumerate(refs):
        assert np.array_equal(fit2["cadence_status"][b], m2["cadence_status"]), b
        good = m2["cadence_status"] == 0
        if good.any():
            worst = max(worst, max(np.max(np.abs(fit2[k][b][good] - m2[k][good])) for k in ("shift_col", "shift_row", "shift_col_err", "shift_row_err")))
    print("the chain's second psf_fit: max |device - mirror| of the shifts and their errors %.3g px" % worst)
    assert worst < 1e-9
    both = (st1[0] == 0) & (fit2["cadence_status"][0] == 0)
    first, second = chi1[0][both].sum(), fit2["chi2"][0][both].sum()
    print("clean cutout, %d cadences: summed chi2 %.1f at the given positions, %.1f at the fitted positions" % (both.sum(), first, second))
    assert both.sum() >= N // 4 and second < first
