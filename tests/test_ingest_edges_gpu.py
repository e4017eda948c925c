"""GPU: the ingest kernels (lightkurve_amd/csrc/ingest.hip) on the synthetic tables and edge shapes of tests/ingest_cases.py,
whose claims tests/test_ingest_cases_cpu.py checks without a GPU.

The FITS decoders only move and convert bytes exactly, and the compaction only moves values: everything is `==` the numpy
reference, NaNs at the same places, zeros with the same sign.  Transit masks are `==` the oracle.  Bins: counts and offsets `==`,
integer-valued targets `==`, general targets within the tolerances tests/test_ingest_gpu.py states (flux 1e-13, errors 1e-12
relative, times 1e-9 d)."""
import ctypes

import numpy as np
import pytest

import ingest_cases as C
from lightkurve_amd import _capi
from test_ingest_gpu import _null_args

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    """Equal values, NaN where the reference has NaN, and the reference's sign on every zero."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(got, want, equal_nan=True), what
    ok = ~np.isnan(want)
    assert np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])), what


def _tables(which):
    if which == "layouts":
        return C.layout_tables()
    if which == "one_empty":
        return (C.make_table("d_e_12", 0),)
    return C.small_tables(int(which.split("_")[1]))


def _unpack(tabs):
    return _capi.fits_unpack_batch([t.raw for t in tabs], [t.desc for t in tabs], [t.bitmask for t in tabs])


# ------------------------------------------------------------------------------------------------ FITS tables
@pytest.mark.parametrize("which", ["layouts", "one_empty", "small_1025", "small_2049"])
def test_fits_unpack_and_cadenceno_over_every_layout_and_batch_shape(which, monkeypatch):
    tabs = _tables(which)
    ref = C.batch_reference(tabs)
    t, f, e, q, off = _unpack(tabs)
    assert np.array_equal(off, ref["new_off"])
    bad = [tabs[b].name for b in range(len(tabs)) for s in [slice(off[b], off[b + 1])]
           if not (np.array_equal(t[s], ref["time"][s], equal_nan=True) and np.array_equal(f[s], ref["flux"][s], equal_nan=True)
                   and np.array_equal(e[s], ref["flux_err"][s], equal_nan=True) and np.array_equal(q[s], ref["quality"][s]))]
    assert not bad, bad
    _same(t, ref["time"], "time"), _same(f, ref["flux"], "flux"), _same(e, ref["flux_err"], "flux_err")
    assert q.dtype == np.int32 and np.array_equal(q, ref["quality"])
    # the integer column of the same tables (J, K, I, B, aligned or not), packed back to back without padding
    c = _capi.fits_cadenceno_batch([x.raw for x in tabs], [x.desc for x in tabs], [x.col for x in tabs],
                                   [x.bitmask for x in tabs], off)
    assert c.dtype == np.int32 and np.array_equal(c, ref["cadenceno"])
    # flux_err_out and quality_out NULL: the same cadences and flux
    _null_args(monkeypatch, "lk_fits_unpack_batch", 8, 9)
    t2, f2, _, _, off2 = _unpack(tabs)
    assert np.array_equal(off2, off)
    _same(t2, ref["time"], "time, bare"), _same(f2, ref["flux"], "flux, bare")


@pytest.mark.parametrize("keep_nan_time", [False, True])
@pytest.mark.parametrize("name", sorted(C.CUBES))
def test_fits_unpack_cube_over_the_cube_cases(name, keep_nan_time):
    c = C.cube_table(name)
    ref = C.cube_reference(c, keep_nan_time)
    t, q, cubes = _capi.fits_unpack_cube(c.raw, c.off_time, c.code_time, c.off_quality, c.code_quality, c.bitmask, keep_nan_time,
                                         c.col_offsets, c.npix)
    assert t.size == ref["keep"].sum() and np.array_equal(t, ref["time"]) and np.array_equal(q, ref["quality"])
    assert cubes.dtype == np.float32
    _same(cubes, ref["cubes"], name)


def test_from_fits_round_trips_synthetic_files(tmp_path):
    from lightkurve_amd.device import DeviceLightCurveBatch
    from lightkurve_amd.ingest import LightCurveBatch
    # E time + I flags at unaligned offsets; K flags and K cadence numbers; a TESS file (the bitmask is an integer for all)
    tabs = [C.make_table("e_i_19", 300, bitmask=0xA8), C.make_table("k_40", 257, bitmask=0xA8), C.make_table("j_24", 513, bitmask=0xA8)]
    paths = []
    for t in tabs:
        paths.append(str(tmp_path / (t.layout + ".fits")))
        C.write_fits(paths[-1], t.rec, t.tforms, telescop="TESS" if t.layout == "j_24" else None)
    ref = C.batch_reference(tabs)
    host = LightCurveBatch.from_fits(paths, quality_bitmask=0xA8)
    dev = DeviceLightCurveBatch.from_fits(paths, quality_bitmask=0xA8)
    assert dev.d_cadenceno is not None
    back = dev.to_host()
    for got in (host, back):
        assert np.array_equal(got.n_off, ref["new_off"]) and np.array_equal(got.quality, ref["quality"])
        _same(got.time, ref["time"]), _same(got.flux, ref["flux"]), _same(got.flux_err, ref["flux_err"])
    assert np.array_equal(back.cadenceno, ref["cadenceno"])
    assert [m["READER_MISSION"] for m in host.meta] == ["generic", "generic", "tess"]


def _unpack_c(raw, raw_off, desc, mask):
    """lk_fits_unpack_batch on a caller-made `raw` / `raw_off` (the wrapper always pads and aligns them)."""
    B = len(mask)
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(B, 10)
    raw_off, mask = np.ascontiguousarray(raw_off, dtype=np.int64), np.ascontiguousarray(mask, dtype=np.int64)
    assert raw.dtype == np.uint8 and raw.size >= raw_off[-1]
    rows = max(int(np.maximum(desc[:, 1], 0).sum()), 1)
    t, f, e = (np.empty(rows) for _ in range(3))
    q, new_off = np.empty(rows, dtype=np.int32), np.zeros(B + 1, dtype=np.int64)
    i64, i32, f64 = (ctypes.POINTER(c) for c in (ctypes.c_int64, ctypes.c_int32, ctypes.c_double))
    _capi._check(_capi._lib.lk_fits_unpack_batch(_capi.Handle.get(0)._h, B, raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                                 raw_off.ctypes.data_as(i64), desc.ctypes.data_as(i32), mask.ctypes.data_as(i64),
                                                 t.ctypes.data_as(f64), f.ctypes.data_as(f64), e.ctypes.data_as(f64),
                                                 q.ctypes.data_as(i32), new_off.ctypes.data_as(i64)))
    return t, f, e, q, new_off


def test_invalid_descriptors_are_refused():
    """Every one of these is turned away by the launcher's argument checks, which come before its first launch: LK_EINVAL ->
    ValueError, and the handle goes on working."""
    tab = C.make_table("j_24", 9)              # 24-byte records: D at 0, E at 8, E at 12, J at 16, J at 20
    ref = C.batch_reference([tab])

    def unpack(raw=tab.raw, **changed):
        desc = tab.desc.copy()
        for k, v in changed.items():
            desc[int(k[1:])] = v
        return _capi.fits_unpack_batch([raw], [desc], [tab.bitmask])

    with pytest.raises(ValueError, match="record length 0 outside"):
        unpack(raw=np.zeros((9, 0), np.uint8), d0=0)
    with pytest.raises(ValueError, match="record length 513 outside"):
        unpack(raw=np.zeros((9, 513), np.uint8), d0=513)
    with pytest.raises(ValueError, match=r"column 1 \(offset 21, type 1\) does not fit the 24-byte record"):
        unpack(d4=21)
    with pytest.raises(ValueError, match=r"column 0 \(offset 17, type 0\) does not fit"):
        unpack(d2=17)
    with pytest.raises(ValueError, match=r"column 3 \(offset 23, type 4\) does not fit"):
        unpack(d8=23, d9=4)
    with pytest.raises(ValueError, match="column 3 has the wrong kind of TFORM"):
        unpack(d9=1)                            # a real code on the flags
    with pytest.raises(ValueError, match="column 0 has the wrong kind of TFORM"):
        unpack(d3=2)                            # an integer code on TIME
    with pytest.raises(ValueError, match="does not fit"):
        unpack(d5=6)                            # no such code
    flat = tab.raw.reshape(-1)
    with pytest.raises(ValueError, match="fewer bytes than rows x record length"):
        _unpack_c(np.concatenate([flat, np.zeros(2, np.uint8)]), [0, flat.size + 2], tab.desc, [tab.bitmask])    # 2 spare bytes, not 3
    two = np.zeros(2 * (flat.size + 6) + 16, np.uint8)
    with pytest.raises(ValueError, match="must start at a multiple of 4 bytes"):
        _unpack_c(two, [0, flat.size + 6, 2 * (flat.size + 6)], [tab.desc, tab.desc], [0, 0])                  # 222 = 2 mod 4
    new_off = ref["new_off"]
    with pytest.raises(ValueError, match=r"integer column \(offset 21, type 2\) does not fit"):
        _capi.fits_cadenceno_batch([tab.raw], [tab.desc], [(21, 2)], [tab.bitmask], new_off)
    with pytest.raises(ValueError, match="integer column"):
        _capi.fits_cadenceno_batch([tab.raw], [tab.desc], [(20, 1)], [tab.bitmask], new_off)       # a real code
    with pytest.raises(ValueError, match="keeps more rows than the table has"):
        _capi.fits_cadenceno_batch([tab.raw], [tab.desc], [tab.col], [tab.bitmask], [0, 10])
    c = C.cube_table("p129_c4_r257_mod3")
    rb = c.raw.shape[1]

    def cube(offsets, npix=c.npix, off_time=c.off_time, code_quality=c.code_quality):
        return _capi.fits_unpack_cube(c.raw, off_time, c.code_time, c.off_quality, code_quality, c.bitmask, True, offsets, npix)

    with pytest.raises(ValueError, match=r"pixel column 3 \(offset %d, 129 pixels\) does not fit" % (rb - 4 * c.npix + 1)):
        cube(c.col_offsets[:3] + [rb - 4 * c.npix + 1])
    with pytest.raises(ValueError, match="pixel column 0"):
        cube([-1])
    with pytest.raises(ValueError, match="bad table description"):
        cube(c.col_offsets + [c.col_offsets[0]])                 # ncols = 5
    with pytest.raises(ValueError, match="TIME does not fit"):
        cube(c.col_offsets, off_time=rb - 7)
    with pytest.raises(ValueError, match="QUALITY does not fit"):
        cube(c.col_offsets, code_quality=1)
    # and the unchanged descriptors decode as before
    t, f, e, q, off = unpack()
    assert np.array_equal(off, new_off) and np.array_equal(t, ref["time"]) and np.array_equal(q, ref["quality"])
    t, f, e, q, off = _unpack_c(np.concatenate([flat, np.zeros(3, np.uint8)]), [0, flat.size + 3], tab.desc, [tab.bitmask])
    k = int(off[1])
    assert np.array_equal(off, new_off) and np.array_equal(f[:k], ref["flux"], equal_nan=True)      # exactly 3 spare bytes do


# ------------------------------------------------------------------------------------------------ remove_nans + normalize
def _medians(flux, n_off):
    return np.array([np.median(v[~np.isnan(v)]) if np.any(~np.isnan(v)) else np.nan
                     for v in (flux[a:b] for a, b in zip(n_off[:-1], n_off[1:]))])


def test_ingest_batch_compaction_at_the_strip_boundaries(monkeypatch):
    names, time, flux, err, n_off = C.compaction_cases()
    keep = ~np.isnan(flux)
    want_off = np.concatenate([[0], np.cumsum(keep)])[n_off]
    med_ref = _medians(flux, n_off)
    assert np.array_equal(med_ref[np.isfinite(med_ref)], [np.nanmedian(flux[a:b]) for a, b, m in zip(n_off[:-1], n_off[1:], med_ref)
                                                          if np.isfinite(m)])
    to, fo, eo, new_off, med = _capi.ingest_batch(time, flux, n_off, flux_err=err, normalize=False)
    assert np.array_equal(new_off, want_off)
    bad = [names[b] for b in range(len(names)) for s, r in [(slice(new_off[b], new_off[b + 1]), slice(n_off[b], n_off[b + 1]))]
           if not (np.array_equal(to[s], time[r][keep[r]]) and np.array_equal(fo[s], flux[r][keep[r]])
                   and np.array_equal(eo[s], err[r][keep[r]], equal_nan=True))]
    assert not bad, bad
    bad = [names[b] for b in np.flatnonzero(~((med == med_ref) | (np.isnan(med) & np.isnan(med_ref))))]
    assert not bad, bad                                          # NaN for the empty and the all-NaN targets
    # without flux_err: the same cadences; e_out, where the caller asks for it, is NaN
    to2, fo2, eo2, new_off2, med2 = _capi.ingest_batch(time, flux, n_off, normalize=False)
    assert eo2 is None and np.array_equal(new_off2, want_off) and np.array_equal(to2, to) and np.array_equal(fo2, fo)
    assert np.array_equal(med2, med, equal_nan=True)
    # normalize: flux / median and err / median bit for bit (by the median the device returned)
    tn, fn, en, new_off3, med3 = _capi.ingest_batch(time, flux, n_off, flux_err=err, normalize=True)
    assert np.array_equal(new_off3, want_off) and np.array_equal(tn, to) and np.array_equal(med3, med, equal_nan=True)
    per = np.repeat(med, np.diff(new_off))
    assert np.array_equal(fn, fo / per) and np.array_equal(en, eo / per, equal_nan=True)
    _null_args(monkeypatch, "lk_ingest_batch", 5)                # flux_err NULL, flux_err_out not
    to4, fo4, eo4, new_off4, _ = _capi.ingest_batch(time, flux, n_off, flux_err=err, normalize=True)
    assert np.array_equal(new_off4, want_off) and np.array_equal(fo4, fn) and np.isnan(eo4).all() and eo4.size == fo4.size


# ------------------------------------------------------------------------------------------------ transit masks
def test_transit_mask_batch_at_tile_edges_and_exact_boundaries():
    m = C.mask_cases()
    got = _capi.transit_mask_batch(m["time"], m["n_off"], m["period"], m["duration"], m["transit_time"], planet_off=m["p_off"])
    assert got.dtype == bool and got.size == m["time"].size
    for b, name in enumerate(m["names"]):
        s = slice(m["n_off"][b], m["n_off"][b + 1])
        assert np.array_equal(got[s], C.mask_reference(m, b)), name
    b = m["names"].index("zero_planets_257")
    assert not got[m["n_off"][b]:m["n_off"][b + 1]].any()
    # full BJD (t / P ~ 1e7): a real mix of True and False, decided by every planet of the target (the CPU test takes each out)
    for name, lo, hi in (("bjd_256_5p", 0.1, 0.9), ("bjd_p03_alone_256_1p", 0.05, 0.5), ("dyadic_257_5p", 0.1, 0.9),
                         ("duration_ge_period_256_1p", 1.0, 1.0), ("duration_zero_255_1p", 0.0, 0.0)):
        b = m["names"].index(name)
        s = slice(m["n_off"][b], m["n_off"][b + 1])
        fin = np.isfinite(m["time"][s])
        assert lo <= got[s][fin].mean() <= hi and not got[s][~fin].any(), name
    for name in ("dyadic_255_1p", "dyadic_1000_1p", "one_on_the_boundary_1p"):      # |phase| == duration / 2 is outside
        b = m["names"].index(name)
        s = slice(m["n_off"][b], m["n_off"][b + 1])
        on, inside = C.dyadic_boundary(np.round(m["time"][s] * 64.0).astype(np.int64))
        assert not got[s][on].any() and got[s][inside].all(), name
    # the C entry point writes the batch's n_off[B] bytes and nothing after them
    ntot = int(m["n_off"][-1])
    buf = np.full(ntot + 256, 0xA5, dtype=np.uint8)
    args = [np.ascontiguousarray(m[k], dtype=np.float64) for k in ("time", "period", "duration", "transit_time")]
    f64, i64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _capi._check(_capi._lib.lk_transit_mask_batch(_capi.Handle.get(0)._h, len(m["names"]), m["n_off"].ctypes.data_as(i64),
                                                  args[0].ctypes.data_as(f64), m["p_off"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  args[1].ctypes.data_as(f64), args[2].ctypes.data_as(f64), args[3].ctypes.data_as(f64),
                                                  buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
    assert np.array_equal(buf[:ntot], got.astype(np.uint8)) and np.all(buf[ntot:] == 0xA5)
    # no planet anywhere in the batch: all False
    none = _capi.transit_mask_batch(m["time"], m["n_off"], np.zeros(0), np.zeros(0), np.zeros(0),
                                    planet_off=np.zeros(len(m["names"]) + 1, np.int32))
    assert not none.any()


# ------------------------------------------------------------------------------------------------ bin
@pytest.mark.parametrize("name", sorted(C.bin_cases()))
def test_bin_batch_on_edges_gaps_and_mixed_errors(name):
    c = C.bin_cases()[name]
    t, f, e, boff = _capi.bin_batch(c["time"], c["flux"], c["n_off"], flux_err=c["flux_err"], time_bin_size=C.BIN_SIZE,
                                    time_bin_start=c["start"])
    refs = [C.bin_reference(c, b) for b in range(len(c["names"]))]
    assert np.array_equal(np.diff(boff), [len(r[0]) for r in refs]) and boff[0] == 0 and t.size == f.size == e.size == boff[-1]
    for b, (target, (rt, rf, re_)) in enumerate(zip(c["names"], refs)):
        s = slice(boff[b], boff[b + 1])
        assert np.allclose(t[s], rt, rtol=0, atol=1e-9), target
        assert np.array_equal(np.isnan(f[s]), np.isnan(rf)) and np.array_equal(np.isnan(e[s]), np.isnan(re_)), target
        if name.startswith("integers"):
            assert np.array_equal(f[s], rf, equal_nan=True) and np.array_equal(e[s], re_, equal_nan=True), target
        else:
            assert np.allclose(f[s], rf, rtol=1e-13, atol=0, equal_nan=True), target
            assert np.allclose(e[s], re_, rtol=1e-12, atol=0, equal_nan=True), target
