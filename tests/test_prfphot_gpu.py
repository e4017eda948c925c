"""GPU: DevicePixelCubeBatch.psf_photometry(prf=) (csrc/prfphot.hip: cube_prfphot_polyphase_kernel, cube_prfphot_images_kernel,
cube_prfphot_kernel<S>, psfphot.hip's status kernel) against the numpy mirror PixelCube.psf_photometry(prf=) on the scenes of
tests/prfphot_cases.py.

Thresholds, named in tests/prfphot_cases.py.  ``C.TILE`` = 16 cadences per workgroup, four lanes each; ``C.N_VALUES`` sits on both
sides of one and of two tiles.  ``C.LDS_ATTR_BYTES`` = 64 KB of LDS per workgroup (``C.lds_bytes``): above it the launcher raises
the kernel's dynamic-LDS attribute first.  With shifts the images of 16 cadences are parked in LDS, so (11, 11) with 4 stars
(86 137 bytes) is the smallest of ``C.SHAPES`` that crosses it and (11, 11) with 8 stars (156 793) sits just under
``C.LDS_MAX_BYTES`` = 160 KiB; without shifts ``C.LDS_CASES`` has (21, 21) with 4 stars (71 385).  ``C.TOO_LARGE`` is refused
before anything is launched, with and without shifts.

Bounds: statuses, n_used, star_off, NaN patterns and shapes exact; flux, flux_err, background and chi2 within 1e-9 max(1, the
cutout's largest |pixel flux|).  test_prfphot_cpu.py shows that no compared cadence has a pivot ratio between 1e-14 and 1e-9, so
no status depends on rounding.  Every comparison prints its largest difference before it asserts (measured on an MI355X: flux
3.1e-14, flux_err 1.8e-15, background 2.3e-15, chi2 1.7e-13)."""

import numpy as np
import pytest

import prfphot_cases as C
import psfphot_cases as G
from lightkurve_amd import _capi, batch
from lightkurve_amd.correctors import PixelCube, TabulatedPRF
from lightkurve_amd.device import DeviceLightCurveBatch, DevicePixelCubeBatch
from lightkurve_amd.devmem import DeviceBuffer, _dp, _i32p, _p, _upload, _vp

pytestmark = pytest.mark.gpu

INFO = (("background", np.float64), ("chi2", np.float64), ("n_used", np.int32), ("cadence_status", np.int8), ("status", np.int32),
        ("star_off", np.int32))


def collect(lcs, info, B, N):
    assert isinstance(lcs, DeviceLightCurveBatch)
    host = lcs.to_host()
    rows = len(lcs)
    assert np.array_equal(host.n_off, np.arange(rows + 1) * N)
    out = dict(flux=host.flux.reshape(rows, N), flux_err=host.flux_err.reshape(rows, N), time=host.time.reshape(rows, N), meta=host.meta)
    for key, dt in INFO:
        a = info[key]
        if isinstance(a, DeviceBuffer):
            a = a.download(dt, {"status": B, "star_off": B + 1}.get(key, B * N), stream=lcs.stream)
        assert a.dtype == dt, key
        out[key] = a.reshape((B, N)) if key not in ("status", "star_off") else a.reshape(-1)
    return out


def run(sc, shifts=False, masked=True, use_flux_err=True, cutouts=None, to_host=True, device_shifts=False, prf=None, prf_index="scene"):
    """psf_photometry(prf=) of the scene's cutouts (or of ``cutouts``, a list of their numbers) with the scene's table and indices
    (or ``prf`` and ``prf_index``, passed as they are) -> dict of host arrays."""
    sel = list(range(sc["B"])) if cutouts is None else list(cutouts)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"][sel], sc["flux"][sel], sc["err"][sel])
    sh = None
    if shifts:
        sh = tuple(np.ascontiguousarray(a[sel]) for a in sc["shifts"])
        if device_shifts:
            sh = tuple(_upload(dev.handle, a, dev.stream, np.float64)[0] for a in sh)
            dev.synchronize()
    lcs, info = dev.psf_photometry(sc["star_col"][sel], sc["star_row"][sel], shifts=sh, aperture_mask=sc["mask"][sel] if masked else "all",
                                   column=C.COLUMN, row=C.ROW, use_flux_err=use_flux_err, to_host=to_host,
                                   prf=prf if prf is not None else C.prf_object(sc["key"]),
                                   prf_index=sc["prf_index"][sel] if isinstance(prf_index, str) else prf_index)
    return collect(lcs, info, len(sel), sc["time"].shape[1])


def bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("flux", "flux_err", "time") + tuple(k for k, _ in INFO))


def check_against_mirror(got, sc, refs, what):
    N = sc["time"].shape[1]
    counts = [len(r["star_index"]) for r in refs]
    assert got["star_off"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert got["flux"].shape == got["flux_err"].shape == got["time"].shape == (sum(counts), N)
    assert got["status"].tolist() == [r["status"] for r in refs], what
    worst = dict(flux=0.0, flux_err=0.0, background=0.0, chi2=0.0)
    for b, ref in enumerate(refs):
        r0, r1 = got["star_off"][b], got["star_off"][b + 1]
        assert np.array_equal(got["cadence_status"][b], ref["cadence_status"]), (what, b, got["cadence_status"][b], ref["cadence_status"])
        assert np.array_equal(got["n_used"][b], ref["n_used"]), (what, b)
        assert np.array_equal(got["time"][r0:r1], np.tile(sc["time"][b], (r1 - r0, 1)), equal_nan=True)
        ok = ref["cadence_status"] == 0
        pairs = (("flux", got["flux"][r0:r1], ref["flux"]), ("flux_err", got["flux_err"][r0:r1], ref["flux_err"]),
                 ("background", got["background"][b], ref["background"]), ("chi2", got["chi2"][b], ref["chi2"]))
        for key, mine, theirs in pairs:
            assert np.array_equal(np.isnan(mine), np.isnan(theirs)) and np.array_equal(np.isnan(theirs), np.broadcast_to(~ok, theirs.shape)), (what, b, key)
        for row, s in zip(range(r0, r1), ref["star_index"]):
            m = got["meta"][row]
            assert m["STAR_INDEX"] == s and m["STAR_COL"] == sc["star_col"][b, s] and m["STAR_ROW"] == sc["star_row"][b, s]
        if not ok.any():
            continue
        scale = max(1.0, float(np.nanmax(np.abs(sc["flux"][b]))))
        for key, mine, theirs in pairs:
            worst[key] = max(worst[key], float(np.max(np.abs(mine[..., ok] - theirs[..., ok]))) / scale)
    print("%s: max |device - mirror| / max(1, the cutout's largest |flux|): flux %.3g, flux_err %.3g, background %.3g, chi2 %.3g"
          % (what, worst["flux"], worst["flux_err"], worst["background"], worst["chi2"]))
    assert max(worst.values()) < 1e-9, (what, worst)


def case_id(c):
    return "%dx%d-S%d-N%d%s%s%s" % (c[0] + c[1:3] + ("-shifts" if c[3] else "", "-masks" if c[4] else "", "" if c[5] else "-unweighted"))


@pytest.mark.parametrize("case", C.GPU_CASES + C.LDS_CASES, ids=case_id)
def test_against_mirror(case):
    shape, S, N, shifts, masked, use_err = case
    sc = C.scene(shape, S, N)
    check_against_mirror(run(sc, shifts, masked, use_err), sc, C.mirror(shape, S, N, shifts, masked, use_err), str(case))


def test_the_cases_cover_what_they_are_meant_to():
    """What the comparison above rests on: every shape with and without shifts and with and without flux_err, the launch paths on
    both sides of the LDS attribute, and scenes that hold each input that can go wrong."""
    for shape, S in C.SHAPES:
        assert {(c[3], c[5]) for c in C.GPU_CASES if c[:2] == (shape, S)} >= {(False, True), (False, False), (True, True), (True, False)}
    sizes = {c: C.lds_bytes(c[0], c[1], c[3], c[5]) for c in C.GPU_CASES + C.LDS_CASES}
    assert C.lds_bytes((11, 11), 4, True) == 86137 and C.lds_bytes((11, 11), 8, True) == 156793 and C.lds_bytes((21, 21), 4, False) == 71385
    assert all(v <= C.LDS_MAX_BYTES for v in sizes.values())
    for shifts in (False, True):
        over = [v for c, v in sizes.items() if c[3] == shifts and v > C.LDS_ATTR_BYTES]
        under = [v for c, v in sizes.items() if c[3] == shifts and v <= C.LDS_ATTR_BYTES]
        assert over and under, shifts
    assert all(C.lds_bytes(shape, S, shifts) > C.LDS_MAX_BYTES for shape, S, shifts in C.TOO_LARGE)
    sc, refs = C.scene((5, 7), 2, 130), C.mirror((5, 7), 2, 130, shifts=True)
    assert np.isnan(sc["flux"][1]).any() and np.isnan(sc["flux"][1, 65]).all() and np.isnan(sc["time"][1]).sum() == 1
    e = sc["err"][1]
    assert (e == 0).any() and np.isnan(e).any() and np.isinf(e).any() and not sc["mask"][1].all()
    assert np.isnan(sc["shifts"][0][1]).sum() == 1 and np.isnan(sc["shifts"][1][1]).sum() == 1
    assert np.isnan(sc["star_col"][2, 0]) and sc["star_col"][2, 1] < C.COLUMN - 0.5 and sc["star_col"][3, 0] == sc["star_col"][3, 1]
    assert sc["prf_index"].tolist() == [0, 1, 0, 1, 0] and C.table(sc["key"])[0].shape[0] == 2
    st = refs[1]["cadence_status"]
    assert (st == 1).sum() == 3 and (st == 2).sum() == 1
    assert all((refs[b]["cadence_status"] == 3).all() and refs[b]["status"] == 1 for b in (3, 4))
    assert refs[2]["star_index"].tolist() == [1] and (refs[2]["cadence_status"] == 0).all()


def test_the_mission_sized_table():
    """os = 50, 551 x 551 (TabulatedPRF.from_gaussian): 2500 phases of 12 x 12, the last sub-image row and column of all but phase
    0 beyond the table."""
    shape, S, N = (11, 11), 4, C.TILE + 1
    sc = C.scene(shape, S, N, "os50")
    prf = C.prf_object("os50")
    zero = np.zeros(sc["B"], dtype=np.int32)
    refs = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_photometry(**dict(C.cutout_arguments(sc, b, True, True), prf=prf, prf_index=0))
            for b in range(sc["B"])]
    check_against_mirror(run(sc, shifts=True, prf=prf, prf_index=zero), sc, refs, "os50 shifts")
    refs = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]).psf_photometry(**dict(C.cutout_arguments(sc, b, False, True), prf=prf, prf_index=0))
            for b in range(sc["B"])]
    check_against_mirror(run(sc, shifts=False, prf=prf, prf_index=None), sc, refs, "os50")


SHAPE, S, N = (11, 11), 4, 33


def test_same_bits_alone_last_in_a_batch_through_a_copy_of_the_table_and_again():
    sc = C.scene(SHAPE, S, N)
    samples, os_ = C.table(sc["key"])
    twice = TabulatedPRF(np.concatenate([samples, samples]), os_)          # tables 2 and 3 are copies of 0 and 1
    for shifts in (False, True):
        whole = run(sc, shifts=shifts)
        assert bits(whole) == bits(run(sc, shifts=shifts)), "two runs differ"
        assert bits(whole) == bits(run(sc, shifts=shifts, prf=twice, prf_index=sc["prf_index"] + 2)), "a copy of the table differs"
        for b in range(sc["B"]):
            alone = run(sc, shifts=shifts, cutouts=[b])
            order = [c for c in range(sc["B"]) if c != b] + [b]
            last = run(sc, shifts=shifts, cutouts=order)
            shared = run(sc, shifts=shifts, cutouts=[b], prf=twice, prf_index=int(sc["prf_index"][b]) + 2)    # a scalar index
            assert bits(shared) == bits(alone), (shifts, b)
            for r, pos in ((whole, b), (last, sc["B"] - 1)):
                r0, r1 = r["star_off"][pos], r["star_off"][pos + 1]
                for key in ("flux", "flux_err", "time"):
                    assert r[key][r0:r1].tobytes() == alone[key].tobytes(), (shifts, b, key)
                for key in ("background", "chi2", "n_used", "cadence_status", "status"):
                    assert r[key][pos].tobytes() == alone[key][0].tobytes(), (shifts, b, key)


def test_shift_forms_to_host_forms_and_the_host_batch_function():
    sc = C.scene(SHAPE, S, N)
    prf = C.prf_object(sc["key"])
    want = run(sc, shifts=True)
    assert bits(run(sc, shifts=True, device_shifts=True)) == bits(want)
    assert bits(run(sc, shifts=True, to_host=False)) == bits(want)
    cubes = [PixelCube(sc["time"][b], sc["flux"][b], sc["err"][b]) for b in range(sc["B"])]
    lcs, info = batch.psf_photometry_batch(cubes, sc["star_col"], sc["star_row"], prf=prf, prf_index=sc["prf_index"], shifts=sc["shifts"],
                                           aperture_mask=sc["mask"], column=C.COLUMN, row=C.ROW)
    assert all(isinstance(info[k], np.ndarray) for k, _ in INFO)
    assert bits(collect(lcs, info, sc["B"], N)) == bits(want)
    assert len(prf._device) == 1                                           # the table went up once and stays with the object


def test_the_gaussian_call_is_untouched():
    """psf_photometry(sigma=) on a scene of psfphot_cases: the same bits before and after a prf= call on the same batch."""
    sc = G.scene((11, 11), 4, 33)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    kw = dict(shifts=sc["shifts"], aperture_mask=sc["mask"], column=G.COLUMN, row=G.ROW)
    before = collect(*dev.psf_photometry(sc["star_col"], sc["star_row"], sc["sigma"], **kw), sc["B"], 33)
    between = collect(*dev.psf_photometry(sc["star_col"], sc["star_row"], prf=C.prf_object("os7"), **kw), sc["B"], 33)
    after = collect(*dev.psf_photometry(sc["star_col"], sc["star_row"], sigma=sc["sigma"], **kw), sc["B"], 33)
    assert bits(before) == bits(after) and bits(between) != bits(before)
    ref = G.mirror((11, 11), 4, 33, shifts=True)
    assert before["cadence_status"].tolist() == [r["cadence_status"].tolist() for r in ref]


def test_a_cutout_beyond_the_lds_limit_is_refused_and_nothing_is_written():
    """C.TOO_LARGE: LK_EINVAL from the launcher's checks, which come before every launch.  Through the C ABI with output buffers
    filled beforehand: they come back as they were."""
    prf = C.prf_object("os4")
    n_prf, Ty, Tx = prf.samples.shape
    for shape, S_, shifts in C.TOO_LARGE:
        ny, nx = shape
        B, N_ = 1, 2
        rng = np.random.default_rng(3)
        flux = (100 + rng.standard_normal((B, N_, ny, nx))).astype(np.float32)
        dev = DevicePixelCubeBatch.from_arrays(np.arange(float(N_))[None], flux, np.ones_like(flux))
        col, row = np.full((B, S_), nx / 2.0) + np.arange(S_), np.full((B, S_), ny / 2.0)
        sh = (np.zeros((B, N_)), np.zeros((B, N_))) if shifts else None
        with pytest.raises(ValueError, match="bytes of LDS"):
            dev.psf_photometry(col, row, prf=prf, shifts=sh)
        h = dev.handle
        fill = np.full(B * S_ * N_, -7.25)
        outs = [_upload(h, fill, dev.stream, np.float64)[0] for _ in range(3)] + [_upload(h, fill[:B * N_], dev.stream, np.float64)[0] for _ in range(2)]
        small = [_upload(h, np.full(B * N_, -7, dtype=np.int32), dev.stream, np.int32)[0], _upload(h, np.full(B * N_, -7, dtype=np.int8), dev.stream, np.int8)[0],
                 _upload(h, np.full(B, -7, dtype=np.int32), dev.stream, np.int32)[0]]
        d_mask, _ = _upload(h, np.ones(ny * nx, dtype=np.uint8), dev.stream, np.uint8)
        d_tab, _ = _upload(h, prf.samples, dev.stream, np.float32)
        d_sh = [_upload(h, a, dev.stream, np.float64)[0] for a in sh] if shifts else [None, None]
        dev.synchronize()
        star_off = np.full(B + 1, -7, dtype=np.int32)
        rc = _capi._lib.lk_cube_prf_photometry_batch_dev(
            h._h, B, N_, ny, nx, _p(dev.d_time), _p(dev.d_flux), _p(dev.d_flux_err), _p(d_mask), 0, S_, col.ctypes.data_as(_dp),
            row.ctypes.data_as(_dp), _p(d_tab), n_prf, Ty, Tx, prf.oversample, None, _p(d_sh[0]), _p(d_sh[1]), 0.0, 0.0, 1,
            star_off.ctypes.data_as(_i32p), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(outs[4]), _p(small[0]), _p(small[1]),
            _p(small[2]), _vp(dev.stream or None))
        assert rc != 0 and np.all(star_off == -7)
        for buf, n in zip(outs, (B * S_ * N_,) * 3 + (B * N_,) * 2):
            assert np.all(buf.download(np.float64, n, stream=dev.stream) == -7.25)
        assert np.all(small[0].download(np.int32, B * N_, stream=dev.stream) == -7) and np.all(small[1].download(np.int8, B * N_, stream=dev.stream) == -7)
        assert np.all(small[2].download(np.int32, B, stream=dev.stream) == -7)
        lcs, info = dev.psf_photometry(col[:, :1], row[:, :1], prf=prf, use_flux_err=False, to_host=True)    # fits, and the batch serves it
        assert info["cadence_status"].tolist() == [[0, 0]] and len(lcs) == 1


def test_arguments_are_checked():
    sc = C.scene((5, 7), 2, 1)
    dev = DevicePixelCubeBatch.from_arrays(sc["time"], sc["flux"], sc["err"])
    prf = C.prf_object(sc["key"])
    col, row, B = sc["star_col"], sc["star_row"], sc["B"]
    for kw in (dict(), dict(sigma=1.0, prf=prf), dict(prf=prf, prf_index=2), dict(prf=prf, prf_index=-1), dict(prf=prf, prf_index=np.zeros(B + 1, dtype=int)),
               dict(prf=prf, prf_index=0.5), dict(sigma=1.0, prf_index=0), dict(prf=np.ones((5, 5))),
               dict(prf=prf, star_col=np.full_like(col, np.nan)), dict(prf=prf, shifts=(np.zeros((B, 2)),) * 2)):
        args = dict(star_col=col, star_row=row)
        args.update(kw)
        with pytest.raises(ValueError):
            dev.psf_photometry(**args)
    # the C ABI's own checks: oversample < 1, n_prf < 1, an index out of range
    h, (n_prf, Ty, Tx) = dev.handle, prf.samples.shape
    d_mask, _ = _upload(h, np.ones(35, dtype=np.uint8), dev.stream, np.uint8)
    d_tab, _ = _upload(h, prf.samples, dev.stream, np.float32)
    outs = [DeviceBuffer(h, B * 2 * 8) for _ in range(8)]
    star = [np.ascontiguousarray(np.where(np.isnan(a), 1.0, a)) for a in (col, row)]
    for tab_args, index in (((n_prf, Ty, Tx, 0), None), ((0, Ty, Tx, 4), None), ((n_prf, Ty, Tx, 4), np.full(B, n_prf, dtype=np.int32)),
                            ((n_prf, Ty, Tx, 4), np.full(B, -1, dtype=np.int32))):
        rc = _capi._lib.lk_cube_prf_photometry_batch_dev(
            h._h, B, 1, 5, 7, _p(dev.d_time), _p(dev.d_flux), _p(dev.d_flux_err), _p(d_mask), 0, 2, star[0].ctypes.data_as(_dp),
            star[1].ctypes.data_as(_dp), _p(d_tab), *tab_args, None if index is None else index.ctypes.data_as(_i32p),
            None, None, C.COLUMN, C.ROW, 1, None, *[_p(b) for b in outs], _vp(dev.stream or None))
        assert rc != 0, (tab_args, index)
    dev.synchronize()
