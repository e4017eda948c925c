"""CPU: the synthetic ingest inputs (tests/ingest_cases.py) are what they claim to be, and the header parser
(lightkurve_amd/fitsio.py) places every column where the builder put it: TFORM codes I / B / K, unaligned offsets, odd record
lengths.  The keep shares and the cadences on bin edges and transit boundaries are conditions on the INPUTS, asserted here on
the references alone; tests/test_ingest_edges_gpu.py then runs the kernels on the same cases."""
import numpy as np
import pytest

import ingest_cases as C
from lightkurve_amd import fitsio
from oracle import np_oracle as O


def test_layout_list_covers_what_it_names():
    tabs = C.layout_tables()
    by_layout = {t.layout: t for t in tabs}
    assert sorted({int(t.desc[0]) for t in tabs}) == [12, 13, 14, 15, 19, 20, 24, 27, 40, 100, 511, 512]
    assert {int(t.desc[1]) for t in tabs} == set(C.ROWS)
    assert {(int(t.desc[3]), int(t.desc[5]), int(t.desc[7])) for t in tabs if t.desc[6] >= 0} >= {
        (0, f, e) for f in (0, 1) for e in (0, 1)}                                          # flux x error as D / E
    assert {int(t.desc[3]) for t in tabs} == {0, 1}                                        # TIME as D and E
    assert any(t.desc[6] < 0 for t in tabs) and any(t.desc[8] < 0 for t in tabs)           # no errors / no flags
    assert {int(t.desc[9]) for t in tabs if t.desc[8] >= 0} == {2, 3, 4, 5}                # flags as J K I B
    for k in (2, 4, 6, 8):                                                                 # every field at 0, 1, 2, 3 mod 4
        assert {int(t.desc[k]) % 4 for t in tabs if t.desc[k] >= 0} == {0, 1, 2, 3}, k
    cad = {(code, off % {2: 4, 3: 8, 4: 2, 5: 1}[code] == 0) for t in by_layout.values() for off, code in [t.col]}
    assert cad >= {(2, True), (2, False), (3, True), (3, False), (4, True), (4, False), (5, True)}
    assert any(t.bitmask < 0 for t in tabs)
    # flags: negative J / I / K, B >= 128, K with bits above 31 (always dropped)
    for layout, test in (("j_24", lambda q: q < 0), ("i_27", lambda q: q < 0), ("k_40", lambda q: q < 0),
                         ("b_e_d_13", lambda q: q >= 128), ("k_100", lambda q: (q >> 32) > 0)):
        t = next(t for t in tabs if t.layout == layout and t.desc[1] == 1300 and t.keep == "share")
        q = t.rec["QUALITY"].astype(np.int64)
        assert test(q).sum() > 10, layout
        kept = C.decode_reference(t.raw, t.desc, t.bitmask)["quality"]
        assert np.all((kept >= -2 ** 31) & (kept < 2 ** 31))          # quality_out is int32
        if layout in ("j_24", "i_27"):
            assert np.all(kept >= 0), layout                # sign-extended negative flags hit bit 40 of the mask
        if layout in ("k_40", "b_e_d_13"):
            assert test(kept).any(), layout                 # kept negative K flags / B flags >= 128 reach quality_out
        if layout == "k_100":
            assert np.any((q >> 32 > 0) & (q & 0xFFFFFFFF == 0))     # high bits alone: a narrowing before the `&` would keep them


def test_value_classes_reach_the_real_columns():
    for t in C.layout_tables():
        if t.desc[1] < 1300 or t.keep != "share":         # (every class many times over: the NaN times overwrite some)
            continue
        for name in ("TIME", "FLUX", "FLUX_ERR"):
            if name not in t.offsets:
                continue
            v = t.rec[name].astype(np.float64)
            tiny = np.finfo(np.float32 if t.letters[name] == "E" else np.float64).tiny
            assert np.any(np.isposinf(v)) and np.any(np.isneginf(v)) and np.any(np.isnan(v)), (t.name, name)
            assert np.any((v == 0) & np.signbit(v)) and np.any((v == 0) & ~np.signbit(v)), (t.name, name)
            assert np.any((v != 0) & (np.abs(v) < tiny)), (t.name, name)           # denormals in the column's own format
            assert np.any(np.abs(v) == np.finfo(t.rec[name].dtype.newbyteorder("=")).max), (t.name, name)


def test_keep_shares():
    tabs = C.layout_tables()
    ref = C.batch_reference(tabs)
    for t, share, n in zip(tabs, ref["kept"], np.diff(ref["new_off"])):
        if t.keep == "all":
            assert n == t.desc[1] > 0, t.name
        elif t.keep == "none":
            assert n == 0 < t.desc[1], t.name
        elif t.keep == "last":
            keep = C.decode_reference(t.raw, t.desc, t.bitmask)["keep"]
            assert n == 1 and keep[-1] and t.desc[1] > 256, t.name
        elif t.desc[1] >= C.SHARE_MIN_ROWS:
            assert 0.25 <= share <= 0.75, (t.name, share)
    for B in (1025, 2049):
        small = C.batch_reference(C.small_tables(B))
        assert 0.25 <= small["new_off"][-1] / (3.0 * B) <= 0.75
        assert {0, 1, 2, 3} == set(np.diff(small["new_off"]))
    # the cube list: row_bytes mod 4, pixels, columns, rows, flag and time types as the builder laid them out
    cubes = [C.cube_table(name) for name in C.CUBES]
    assert {c.raw.shape[1] % 4 for c in cubes} == {0, 1, 2, 3}
    assert {c.npix for c in cubes} == {1, 127, 128, 129, 400} and {len(c.col_offsets) for c in cubes} == {1, 2, 3, 4}
    assert {c.rec.size for c in cubes} == {1, 255, 256, 257, 600}
    assert {c.code_quality for c in cubes} == {2, 4} and {c.code_time for c in cubes} == {0, 1}
    for c in cubes:        # both branches of the cube kernel: rows whose first pixel sits at a multiple of 4 bytes, and rows where not
        at = (np.arange(c.rec.size)[:, None] * c.raw.shape[1] + np.array(c.col_offsets)[None, :]) % 4
        if c.rec.size >= 255 and c.bitmask != -1:
            assert (at != 0).any(), c.name
            assert (at == 0).any() or c.name == "p400_c1_r600_mod0_skewed", c.name
    for name in C.CUBES:
        c = C.cube_table(name)
        t = c.rec["TIME"].astype(np.float64)
        if c.rec.size >= 255:
            assert np.isnan(t).any() and np.isinf(t).any(), name
        for keep_nan_time in (False, True):
            r = C.cube_reference(c, keep_nan_time)
            assert r["cubes"].shape == (len(c.col_offsets), r["keep"].sum(), c.npix) and np.isfinite(r["time"]).all()
            if c.bitmask == -1:
                assert r["keep"].sum() == 0
            else:          # every other case reaches the cube kernel; the NaN-time row only when NaN times are kept
                assert r["keep"].sum() >= 1 or (name == "p1_c1_r1_nan_time" and not keep_nan_time), (name, keep_nan_time)
            if name in C.ONE_ROW and r["keep"].sum():
                assert r["cubes"].shape == (1, 1, 1) and r["cubes"][0, 0, 0] == np.float32(C.ONE_ROW[name][1]) != 0
                assert r["time"][0] == (0.0 if name == "p1_c1_r1_nan_time" else C.ONE_ROW[name][0])
            elif c.rec.size >= 255 and c.bitmask != -1:
                assert 0.25 <= r["keep"].mean() <= 0.75, (name, keep_nan_time)
        if c.rec.size >= 255 and c.bitmask != -1:
            assert C.cube_reference(c, True)["keep"].sum() > C.cube_reference(c, False)["keep"].sum()
            assert np.any(C.cube_reference(c, True)["time"] == 0.0)


@pytest.mark.parametrize("layout", sorted(C.LAYOUTS))
def test_written_files_parse_to_the_builders_layout(tmp_path, layout):
    t = C.make_table(layout, 257)
    path = str(tmp_path / (layout + ".fits"))
    C.write_fits(path, t.rec, t.tforms, telescop="TESS" if layout == "j_24" else None)
    tab = fitsio.read_fits_table(path)
    assert tab.n_rows == 257 and tab.row_bytes == t.desc[0] and np.array_equal(tab.raw, t.raw)
    desc, bitmask, mission = fitsio.lightcurve_columns(tab, quality_bitmask=t.bitmask)
    assert np.array_equal(desc, t.desc) and mission == ("tess" if layout == "j_24" else "generic")
    assert bitmask == t.bitmask
    if "CADENCENO" in t.offsets:
        assert fitsio.int_column(tab) == t.col
    else:
        assert fitsio.int_column(tab) is None
    if "QUALITY" in t.offsets:
        assert fitsio.int_column(tab, "quality") == (t.offsets["QUALITY"], C.CODES[t.letters["QUALITY"]])
    ref = C.decode_reference(tab.raw, desc, bitmask, col=t.col)
    assert ref["time"].size == ref["keep"].sum() == ref["cadenceno"].size


def test_integer_scalar_columns_of_every_code_are_accepted_and_scaled_or_vector_columns_refused(tmp_path):
    rng = np.random.default_rng(5)
    for letter in "IBKJ":
        fields = [("PAD0", "B", 1), ("TIME", "D", 1), ("FLUX", "E", 1), ("QUALITY", letter, 1), ("PAD1", "B", 2), ("CADENCENO", letter, 1)]
        rec, raw, offs = C.fits_table(fields, 9, rng)
        path = str(tmp_path / ("int_%s.fits" % letter))
        C.write_fits(path, rec, ["%d%s" % (r, lt) for _, lt, r in fields])
        tab = fitsio.read_fits_table(path)
        desc, _, _ = fitsio.lightcurve_columns(tab)
        assert tuple(desc[8:]) == (offs["QUALITY"], C.CODES[letter]) and desc[6] == -1
        assert fitsio.int_column(tab) == (offs["CADENCENO"], C.CODES[letter])
    fields = [("TIME", "D", 1), ("FLUX", "E", 1), ("QUALITY", "J", 1), ("CADENCENO", "J", 1)]
    rec, raw, offs = C.fits_table(fields, 4, rng)
    forms = ["1D", "1E", "1J", "1J"]
    for i, name in ((1, "TIME"), (2, "FLUX"), (3, "QUALITY")):
        path = str(tmp_path / ("scaled_%d.fits" % i))
        C.write_fits(path, rec, forms, cards=[("TSCAL%d" % i, 2.0)])
        with pytest.raises(NotImplementedError, match="scaled"):
            fitsio.lightcurve_columns(fitsio.read_fits_table(path))
    path = str(tmp_path / "scaled_cad.fits")
    C.write_fits(path, rec, forms, cards=[("TZERO4", 32768)])
    assert fitsio.int_column(fitsio.read_fits_table(path)) is None
    rec, raw, offs = C.fits_table([("TIME", "D", 2), ("FLUX", "E", 1)], 4, rng)
    path = str(tmp_path / "vector_time.fits")
    C.write_fits(path, rec, ["2D", "1E"])
    with pytest.raises(NotImplementedError, match="TFORM 2D"):
        fitsio.lightcurve_columns(fitsio.read_fits_table(path))
    # a real code where an integer belongs, and the other way round
    rec, raw, offs = C.fits_table([("TIME", "J", 1), ("FLUX", "E", 1), ("QUALITY", "E", 1)], 4, rng)
    path = str(tmp_path / "kinds.fits")
    C.write_fits(path, rec, ["1J", "1E", "1E"])
    with pytest.raises(NotImplementedError):
        fitsio.lightcurve_columns(fitsio.read_fits_table(path))


@pytest.mark.parametrize("name", sorted(C.CUBES))
def test_cube_files_parse_to_the_builders_layout(tmp_path, name):
    c = C.cube_table(name)
    rec = c.rec.copy()
    cols = ["FLUX", "FLUX_ERR", "FLUX_BKG", "FLUX_BKG_ERR"][:len(c.col_offsets)]
    rec.dtype.names = tuple({"PIX%d" % i: n for i, n in enumerate(cols)}.get(n, n) for n in rec.dtype.names)
    path = str(tmp_path / (name + ".fits"))
    C.write_fits(path, rec, c.tforms)
    tab = fitsio.read_fits_table(path)
    pc = fitsio.pixel_columns(tab, columns=tuple(n.lower() for n in cols), quality_bitmask=c.bitmask)
    assert np.array_equal(tab.raw, c.raw)
    assert (pc["off_time"], pc["code_time"], pc["off_quality"], pc["code_quality"]) == (c.off_time, c.code_time, c.off_quality,
                                                                                         c.code_quality)
    assert pc["col_offsets"] == c.col_offsets and pc["npix"] == c.npix and pc["bitmask"] == c.bitmask and pc["keep_nan_time"]


def test_compaction_cases_sit_on_the_strip_boundaries():
    names, time, flux, err, n_off = C.compaction_cases()
    assert len(names) == len(C.COMPACT_N) * len(C.COMPACT_PATTERNS) and set(np.diff(n_off)) == set(C.COMPACT_N)
    kept = np.array([np.count_nonzero(~np.isnan(flux[a:b])) for a, b in zip(n_off[:-1], n_off[1:])])
    n = np.diff(n_off)
    empty = np.flatnonzero(kept == 0)
    assert np.any(n[empty] > 0) and np.any(n[empty] == 0)
    for size in (0, 4097):                                       # an empty and an all-NaN target between ordinary ones
        assert any(n[b] == size and kept[b - 1] > 0 and kept[b] == 0 and kept[b + 1] > 0 for b in range(1, len(n) - 1)), size
    strip = C.nan_pattern("strip", 4097)
    assert strip[576:1152].all() and strip.sum() == 576          # 4097 cadences: strips of 576, the second one NaN
    assert C.nan_pattern("strip", 513)[128:256].all() and C.nan_pattern("strip", 65)[64] and C.nan_pattern("strip", 64).all()


def test_dyadic_mask_targets_have_cadences_on_the_boundary_and_the_reference_excludes_them():
    m = C.mask_cases()
    assert sorted(set(np.diff(m["n_off"]))) == [0, 1, 255, 256, 257, 1000] and sorted(set(np.diff(m["p_off"]))) == [0, 1, 5]
    # every planet of a five-planet target decides cadences of its own: without it the reference changes, and the mask is mixed
    for name in ("bjd_256_5p", "dyadic_257_5p"):
        b = m["names"].index(name)
        t = m["time"][m["n_off"][b]:m["n_off"][b + 1]]
        ps = np.arange(m["p_off"][b], m["p_off"][b + 1])
        ref = C.mask_reference(m, b)
        fin = np.isfinite(t)
        assert 0.1 < ref[fin].mean() < 0.9 and not ref[~fin].any(), name
        with np.errstate(invalid="ignore"):
            for p in ps:
                rest = ps[ps != p]
                less = O.transit_mask(t, m["period"][rest], m["duration"][rest], m["transit_time"][rest])
                assert np.count_nonzero(less != ref) >= 2, (name, p)
    seen = 0
    for name, k0 in (("dyadic_255_1p", 0), ("dyadic_1000_1p", 0), ("one_on_the_boundary_1p", None)):
        b = m["names"].index(name)
        t = m["time"][m["n_off"][b]:m["n_off"][b + 1]]
        k = t * 64.0
        assert np.array_equal(k, np.round(k))
        on, inside = C.dyadic_boundary(k.astype(np.int64))
        assert on.sum() > 0, name
        ref = C.mask_reference(m, b)
        assert not ref[on].any() and np.array_equal(ref, inside), name
        seen += int(on.sum())
    assert seen >= 10
    b = m["names"].index("zero_planets_257")
    assert not C.mask_reference(m, b).any()
    b = m["names"].index("bjd_256_5p")
    t = m["time"][m["n_off"][b]:m["n_off"][b + 1]]
    assert np.nanmin(np.abs(t[np.isfinite(t)])) / 0.3 > 7e6 and np.isnan(t).any() and np.isinf(t).sum() == 2
    for name, lo, hi in (("bjd_p03_alone_256_1p", 0.05, 0.5), ("duration_ge_period_256_1p", 1.0, 1.0),
                         ("duration_zero_255_1p", 0.0, 0.0)):
        b = m["names"].index(name)
        tb = m["time"][m["n_off"][b]:m["n_off"][b + 1]]
        ref = C.mask_reference(m, b)
        assert lo <= ref[np.isfinite(tb)].mean() <= hi and not ref[~np.isfinite(tb)].any(), name
    b = m["names"].index("duration_zero_255_1p")
    assert np.any((m["time"][m["n_off"][b]:m["n_off"][b + 1]] - 1.0) % 2.0 == 0.0)        # cadences at phase 0 exactly
    assert (m["period"] < 0).any() and (m["duration"] == 0).any() and (m["duration"] >= np.abs(m["period"])).any()


def test_dyadic_bin_targets_have_cadences_on_the_edges_and_the_reference_follows_the_rule():
    cases = C.bin_cases()
    c = cases["integers"]
    b = c["names"].index("int_span_3d")
    s = slice(c["n_off"][b], c["n_off"][b + 1])
    k = np.round(c["time"][s] * 64.0).astype(np.int64)
    assert np.array_equal(k / 64.0, c["time"][s]) and k[-1] == 192
    assert np.count_nonzero(k % 16 == 0) == 13                   # cadences exactly on an edge
    rt, rf, re_ = C.bin_reference(c, b)
    assert len(rt) == 12                                         # 3.0 d at 0.25 d: the cadence on the last edge is dropped
    f = c["flux"][s]
    with np.errstate(all="ignore"):
        for j in range(12):                                      # (edges[j], edges[j + 1]], and 0 goes to bin 0
            sel = ((k > 16 * j) & (k <= 16 * (j + 1)) | ((k == 0) & (j == 0))) & (k < 192)
            want = np.nansum(f[sel]) / np.count_nonzero(~np.isnan(f[sel])) if np.any(~np.isnan(f[sel])) else np.nan
            assert np.array_equal(rf[j], want, equal_nan=True), j
    assert np.isnan(rf[1]) and re_[1] == 2.0 and np.all(re_ == 2.0)
    assert np.array_equal(rt, 0.125 + 0.25 * np.arange(12))
    # the whole list: sizes, totals, targets without bins between others, starts on both sides of the first cadence
    g = cases["general"]
    nb = [len(C.bin_reference(g, b)[0]) for b in range(len(g["names"]))]
    assert sum(nb) > 256 and max(nb) > 256 and set(np.diff(g["n_off"])) >= {0, 1}
    assert any(nb[b] == 0 and nb[b - 1] > 0 and nb[b + 1] > 0 for b in range(1, len(nb) - 1))
    b = g["names"].index("gap_nan_err")
    rt, rf, re_ = C.bin_reference(g, b)
    assert np.isnan(rf).sum() > 390 and np.isfinite(re_).any()                   # the gap's bins; nanstd where there is flux
    b = g["names"].index("duplicates_partial_err")
    s = slice(g["n_off"][b], g["n_off"][b + 1])
    assert np.any(np.diff(g["time"][s]) == 0) and np.isinf(g["flux_err"][s]).any() and np.isnan(g["flux_err"][s]).any()
    rt, rf, re_ = C.bin_reference(g, b)
    assert np.isinf(re_).any() and np.isnan(re_).any() and np.isfinite(re_).any()
    b = g["names"].index("nan_flux_bin_no_err")
    assert np.isnan(C.bin_reference(g, b)[1][2])
    for name in ("start_before", "start_after", "start_per_target", "integers_start_after"):
        c = cases[name]
        first = np.array([c["time"][a] if e > a else np.nan for a, e in zip(c["n_off"][:-1], c["n_off"][1:])])
        start = np.broadcast_to(c["start"], first.shape)
        if name != "start_before":
            assert np.any(start > first)
        if name != "start_after" and name != "integers_start_after":
            assert np.any(start < first)
    nb = [len(C.bin_reference(cases["start_per_target"], b)[0]) for b in range(len(g["names"]))]
    assert nb[-1] == 0 and nb[0] > 0
    assert len(C.bin_reference(cases["start_before"], g["names"].index("one_cadence"))[0]) == 3
