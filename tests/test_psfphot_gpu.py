"""GPU: DevicePixelCubeBatch.psf_photometry (csrc/psfphot.hip: cube_psfphot_tables_kernel, cube_psfphot_kernel<S>,
cube_psfphot_status_kernel) against the numpy mirror PixelCube.psf_photometry on the scenes of tests/psfphot_cases.py.

Three thresholds, named in tests/psfphot_cases.py.  ``C.TILE`` = 16: a workgroup takes a tile of 16 cadences, four lanes each
(lane k of a cadence walks the pixel rows k, k + 4, ...); ``C.N_VALUES`` sits on both sides of one and of two tiles (15, 16, 17,
31, 32, 33) next to 1, 63, 64, 65 and 130.  ``C.LDS_ATTR_BYTES`` = 64 KB of LDS per workgroup (a function of shape, star count
and shifts, ``C.lds_bytes``): above it the launcher raises the kernel's dynamic-LDS attribute first; ``C.LDS_CASES`` has (21, 21)
with 4 stars below it (no shifts) and above it (shifts).  ``C.LDS_MAX_BYTES`` = 160 KiB: (35, 35) with one star sits just under
it, ``C.TOO_LARGE`` = (36, 36) beyond it and is refused with ValueError before anything is launched.  The other shapes differ in
what they exercise: (3, 3) one star and fewer rows than lanes per cadence, (5, 7) not square, (11, 11) with 4 and with 8 stars,
(13, 17) 221 pixels.

Bounds: statuses, n_used, NaN patterns and shapes exact; flux and background 1e-9 of the cutout's largest |flux| (the house rule
for float64 sums in another order: the device adds four interleaved groups of pixel rows with fused multiply-adds, numpy's
einsum in blocks); flux_err 1e-9 relative; chi2 1e-9 of sum w y^2, the scale of the terms that cancel in it.
test_psfphot_cpu.py shows that no compared cadence has a pivot ratio between 1e-14 and 1e-9, so no status depends on rounding.
Every comparison prints its largest difference before it asserts (measured on an MI355X: flux 1.8e-14, background 1.1e-15,
flux_err 1.8e-14, chi2 1.2e-16)."""
import functools

import numpy as np
import pytest

import psfphot_cases as C
from lightkurve_amd import batch
from lightkurve_amd.correctors import PixelCube
from lightkurve_amd.device import DeviceLightCurveBatch, DevicePixelCubeBatch
from lightkurve_amd.devmem import DeviceBuffer, _upload

pytestmark = pytest.mark.gpu

INFO = (("background", np.float64), ("chi2", np.float64), ("n_used", np.int32), ("cadence_status", np.int8), ("status", np.int32),
        ("star_off", np.int32))


def run(sc, shifts=False, masked=True, use_flux_err=True, cutouts=None, to_host=True, device_shifts=False):
    """psf_photometry of the scene's cutouts (or of ``cutouts``, a list of their numbers) -> dict of host arrays: flux, flux_err,
    time (rows, N), the keys of INFO, and meta."""
    sel = list(range(sc["B"])) if cutouts is None else list(cutouts)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"][sel], sc["flux"][sel], sc["err"][sel])
    sh = None
    if shifts:
        sh = tuple(np.ascontiguousarray(a[sel]) for a in sc["shifts"])
        if device_shifts:
            sh = tuple(_upload(dev.handle, a, dev.stream, np.float64)[0] for a in sh)
            dev.synchronize()
    lcs, info = dev.psf_photometry(sc["star_col"][sel], sc["star_row"][sel], sc["sigma"][sel], shifts=sh,
                                   aperture_mask=sc["mask"][sel] if masked else "all", column=C.COLUMN, row=C.ROW,
                                   use_flux_err=use_flux_err, to_host=to_host)
    return collect(lcs, info, len(sel), sc["time"].shape[1])


def collect(lcs, info, B, N):
    assert isinstance(lcs, DeviceLightCurveBatch)
    host = lcs.to_host()
    rows = len(lcs)
    assert np.array_equal(host.n_off, np.arange(rows + 1) * N)
    out = dict(flux=host.flux.reshape(rows, N), flux_err=host.flux_err.reshape(rows, N), time=host.time.reshape(rows, N), meta=host.meta)
    for key, dt in INFO:
        a = info[key]
        if isinstance(a, DeviceBuffer):
            count = {"status": B, "star_off": B + 1}.get(key, B * N)
            a = a.download(dt, count, stream=lcs.stream)
        assert a.dtype == dt, key
        out[key] = a.reshape((B, N)) if a.size == B * N and key not in ("status", "star_off") else a.reshape(-1)
    return out


@functools.lru_cache(maxsize=None)
def device_result(case):
    shape, S, N, shifts, masked, use_err = case
    return run(C.scene(shape, S, N), shifts, masked, use_err)


def bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("flux", "flux_err", "time") + tuple(k for k, _ in INFO))


def check_against_mirror(got, sc, refs, what, use_flux_err=True, masked=True):
    B, N = sc["B"], sc["time"].shape[1]
    counts = [len(r["star_index"]) for r in refs]
    assert got["star_off"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert got["flux"].shape == got["flux_err"].shape == got["time"].shape == (sum(counts), N)
    assert got["status"].tolist() == [r["status"] for r in refs], what
    worst = dict(flux=0.0, background=0.0, flux_err=0.0, chi2=0.0)
    for b, ref in enumerate(refs):
        r0, r1 = got["star_off"][b], got["star_off"][b + 1]
        assert np.array_equal(got["cadence_status"][b], ref["cadence_status"]), (what, b, got["cadence_status"][b], ref["cadence_status"])
        assert np.array_equal(got["n_used"][b], ref["n_used"]), (what, b)
        assert np.array_equal(got["time"][r0:r1], np.tile(sc["time"][b], (r1 - r0, 1)), equal_nan=True)
        ok = ref["cadence_status"] == 0
        for key, mine, theirs in (("flux", got["flux"][r0:r1], ref["flux"]), ("flux_err", got["flux_err"][r0:r1], ref["flux_err"]),
                                  ("background", got["background"][b], ref["background"]), ("chi2", got["chi2"][b], ref["chi2"])):
            assert np.array_equal(np.isnan(mine), np.isnan(theirs)) and np.array_equal(np.isnan(theirs), np.broadcast_to(~ok, theirs.shape)), (what, b, key)
        for row, s in zip(range(r0, r1), ref["star_index"]):
            m = got["meta"][row]
            assert m["STAR_INDEX"] == s and m["STAR_COL"] == sc["star_col"][b, s] and m["STAR_ROW"] == sc["star_row"][b, s]
        if not ok.any():
            continue
        top = np.max(np.abs(ref["flux"][:, ok]))
        y = sc["flux"][b].reshape(N, -1).astype(np.float64)
        e = sc["err"][b].reshape(N, -1).astype(np.float64)
        used = (sc["mask"][b].reshape(-1) if masked else np.ones(y.shape[1], dtype=bool))[None, :] & np.isfinite(y)
        if use_flux_err:
            used &= np.isfinite(e) & (e > 0)
        with np.errstate(all="ignore"):
            wy2 = np.sum(np.where(used, y * y / (e * e if use_flux_err else 1.0), 0.0), axis=1)
        d = dict(flux=np.max(np.abs(got["flux"][r0:r1][:, ok] - ref["flux"][:, ok])) / top,
                 background=np.max(np.abs(got["background"][b][ok] - ref["background"][ok])) / top,
                 flux_err=np.max(np.abs(got["flux_err"][r0:r1][:, ok] / ref["flux_err"][:, ok] - 1.0)),
                 chi2=np.max(np.abs(got["chi2"][b][ok] - ref["chi2"][ok]) / wy2[ok]))
        for key in worst:
            worst[key] = max(worst[key], d[key])
    print("%s: max |device - mirror|: flux %.3g, background %.3g of the largest flux; flux_err %.3g relative; chi2 %.3g of sum w y^2"
          % (what, worst["flux"], worst["background"], worst["flux_err"], worst["chi2"]))
    assert max(worst.values()) < 1e-9, (what, worst)


@pytest.mark.parametrize("case", C.GPU_CASES, ids=lambda c: "%dx%d-S%d-N%d%s%s%s" % (c[0] + c[1:3] + ("-shifts" if c[3] else "", "-masks" if c[4] else "",
                                                                                                    "" if c[5] else "-unweighted")))
def test_against_mirror(case):
    shape, S, N, shifts, masked, use_err = case
    check_against_mirror(device_result(case), C.scene(shape, S, N), C.mirror(shape, S, N, shifts, masked, use_err), str(case), use_err, masked)


def test_every_bad_input_is_in_the_scenes():
    """What the comparison above rests on: the scenes do contain each input that can go wrong, and each status arises."""
    sc, refs = C.scene((5, 7), 2, 130), C.mirror((5, 7), 2, 130, shifts=True)
    assert np.isnan(sc["flux"][1]).any() and np.isnan(sc["flux"][1, 65]).all() and np.isnan(sc["time"][1]).sum() == 1
    e = sc["err"][1]
    assert (e == 0).any() and np.isnan(e).any() and np.isinf(e).any() and not sc["mask"][1].all()
    assert np.isnan(sc["shifts"][0][1]).sum() == 1 and np.isnan(sc["shifts"][1][1]).sum() == 1
    assert np.isnan(sc["star_col"][2, 0]) and np.isnan(sc["star_col"][2]).sum() == 1 and sc["star_col"][2, 1] < C.COLUMN - 0.5
    assert sc["star_col"][3, 0] == sc["star_col"][3, 1] and len(set(map(tuple, sc["sigma"]))) == sc["B"]
    st = refs[1]["cadence_status"]
    assert (st == 1).sum() == 3 and (st == 2).sum() == 1 and (refs[3]["cadence_status"] == 3).all() and refs[3]["status"] == 1
    assert refs[2]["flux"].shape[0] == 1 and refs[2]["star_index"].tolist() == [1] and (refs[2]["cadence_status"] == 0).all()
    wide = C.scene((11, 11), 8, 130)                                # the padding in front of seven stars: rows 0 .. 6 are slots 1 .. 7
    assert np.isnan(wide["star_col"][2, 0]) and not np.isnan(wide["star_col"][2, 1:]).any()


def test_the_lds_cases_sit_where_they_are_meant_to():
    (under, over, top), (big, big_s) = C.LDS_CASES, C.TOO_LARGE
    assert C.lds_bytes(under[0], under[1], under[3]) == 58617 < C.LDS_ATTR_BYTES < C.lds_bytes(over[0], over[1], over[3]) == 78777
    assert C.LDS_ATTR_BYTES < C.lds_bytes(top[0], top[1], top[3]) == 158969 <= C.LDS_MAX_BYTES < C.lds_bytes(big, big_s, False) == 168272
    assert all(C.lds_bytes(c[0], c[1], c[3], c[5]) < C.LDS_ATTR_BYTES for c in C.GPU_CASES if c not in (over, top))


def test_a_cutout_beyond_the_lds_limit_is_refused():
    """(36, 36) needs 168 272 bytes of LDS > LDS_MAX_BYTES: LK_EINVAL -> ValueError from the launcher's checks, which come before
    every launch; the output buffers of the call are never written (nothing to compare), and the batch serves the next call."""
    shape, S = C.TOO_LARGE
    ny, nx = shape
    rng = np.random.default_rng(3)
    flux = (100 + rng.standard_normal((1, 2, ny, nx))).astype(np.float32)
    dev = DevicePixelCubeBatch.from_arrays(np.arange(2.0)[None], flux, np.ones_like(flux))
    with pytest.raises(ValueError, match="bytes of LDS"):
        dev.psf_photometry([nx / 2], [ny / 2], 1.5)
    with pytest.raises(ValueError, match="bytes of LDS"):
        dev.psf_photometry([nx / 2], [ny / 2], 1.5, shifts=(np.zeros((1, 2)), np.zeros((1, 2))))
    lcs, info = dev.psf_photometry([nx / 2], [ny / 2], 1.5, use_flux_err=False, to_host=True)     # 85 072 bytes: fits, and runs
    assert info["cadence_status"].tolist() == [[0, 0]] and len(lcs) == 1


SHAPE, S, N = (11, 11), 4, 130


def test_same_bits_alone_in_the_batch_and_elsewhere():
    sc = C.scene(SHAPE, S, N)
    for shifts in (False, True):
        whole = run(sc, shifts=shifts)
        again = run(sc, shifts=shifts)
        assert bits(whole) == bits(again), "two runs differ"
        order = [2, 0, 3, 1]
        moved = run(sc, shifts=shifts, cutouts=order)
        for b in range(sc["B"]):
            alone = run(sc, shifts=shifts, cutouts=[b])
            at = order.index(b)
            for r, pos in ((whole, b), (moved, at)):
                r0, r1 = r["star_off"][pos], r["star_off"][pos + 1]
                for key in ("flux", "flux_err", "time"):
                    assert r[key][r0:r1].tobytes() == alone[key].tobytes(), (shifts, b, key)
                for key in ("background", "chi2", "n_used", "cadence_status", "status"):
                    assert r[key][pos].tobytes() == alone[key][0].tobytes(), (shifts, b, key)


def test_to_host_forms_shift_forms_and_the_host_batch_function():
    sc = C.scene(SHAPE, S, N)
    want = run(sc, shifts=True)
    assert bits(run(sc, shifts=True, to_host=False)) == bits(want)
    assert bits(run(sc, shifts=True, device_shifts=True)) == bits(want)
    cubes = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]) for b in range(sc["B"])]
    lcs, info = batch.psf_photometry_batch(cubes, sc["star_col"], sc["star_row"], sc["sigma"], shifts=sc["shifts"], aperture_mask=sc["mask"],
                                           column=C.COLUMN, row=C.ROW)
    assert all(isinstance(info[k], np.ndarray) for k, _ in INFO)
    assert bits(collect(lcs, info, sc["B"], N)) == bits(want)
    # one star list for every cutout ([S]) and one sigma pair = the same, written out per cutout
    col, row = sc["star_col"][0], sc["star_row"][0]
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    a = collect(*dev.psf_photometry(col, row, (1.1, 0.9), column=C.COLUMN, row=C.ROW), sc["B"], N)
    b = collect(*dev.psf_photometry(np.tile(col, (sc["B"], 1)), np.tile(row, (sc["B"], 1)), np.tile([1.1, 0.9], (sc["B"], 1)),
                                    column=C.COLUMN, row=C.ROW), sc["B"], N)
    assert bits(a) == bits(b)


def test_arguments_are_checked():
    sc = C.scene((5, 7), 2, 1)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    col, row = sc["star_col"], sc["star_row"]
    for kw in (dict(sigma=0.0), dict(sigma=np.nan), dict(star_col=np.full_like(col, np.nan)), dict(star_col=np.tile(col, (1, 5)), star_row=np.tile(row, (1, 5))),
               dict(shifts=(np.zeros((sc["B"], 2)),) * 2), dict(shifts=(np.zeros((sc["B"], 1)),)), dict(star_col=np.where(np.isnan(col), np.nan, np.inf))):
        args = dict(star_col=col, star_row=row, sigma=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            dev.psf_photometry(**args)


def test_chain_finds_the_star_with_the_transit():
    """Two blended stars 1.7 px apart; star 1 carries a box transit, star 0 does not: psf_photometry -> remove_nans -> normalize
    -> bls puts star 1's peak at the injected period, and star 0's depth stays below a third of star 1's."""
    shape, N, period, depth, dur = (11, 11), 1500, 2.5, 0.02, 0.15
    rng = np.random.default_rng(11)
    time = 2000.0 + np.arange(N) * 0.01
    col, row, sig = np.array([4.2, 5.9]), np.array([5.1, 5.3]), 1.1
    in_transit = np.abs((time - 2000.7 + period / 2) % period - period / 2) < dur / 2
    f = np.stack([np.full(N, 6000.0), 4000.0 * np.where(in_transit, 1 - depth, 1.0)])
    img = 30.0 + sum(f[s][:, None, None] * C.psf_image(shape, col[s], row[s], sig, sig)[None] for s in range(2))
    err = np.sqrt(img / 25.0)
    flux = (img + err * rng.standard_normal(img.shape)).astype(np.float32)
    flux[700] = np.nan                                                      # one failed cadence: remove_nans drops it
    dev = DevicePixelCubeBatch.from_arrays(time[None], flux[None], err.astype(np.float32)[None])
    lcs, info = dev.psf_photometry(col, row, sig, to_host=True)
    assert info["cadence_status"][0, 700] == 2 and (info["cadence_status"] == 0).sum() == N - 1
    clean = lcs.remove_nans().normalize()
    assert np.diff(clean.n_off).tolist() == [N - 1, N - 1]
    periods = np.linspace(1.5, 3.5, 401)
    pk = clean.bls(periods, duration=[dur]).peaks()
    print("BLS peaks: period %s, depth %s" % (pk["period"], pk["depth"]))
    assert abs(pk["period"][1] - period) <= 0.005 + 1e-12
    assert 0.5 * depth < pk["depth"][1] < 1.5 * depth and abs(pk["depth"][0]) < pk["depth"][1] / 3
