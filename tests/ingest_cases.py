"""Synthetic inputs and numpy references for the ingest kernels (lightkurve_amd/csrc/ingest.hip): FITS tables of every
layout the decoders accept, pixel cubes, NaN patterns for the remove_nans compaction, transit-mask and bin edge cases.  No
GPU here: tests/test_ingest_cases_cpu.py checks the builders and references on their own, tests/test_ingest_edges_gpu.py runs
the kernels on them.

The FITS reference is numpy decoding the same big-endian bytes (`decode` of tests/test_fitsio_cpu.py, extended below): every
step is an exact conversion, so the comparisons are `==`.  Transit masks and bins go through oracle/np_oracle.py."""
import functools
import types
import zlib

import numpy as np

from oracle import np_oracle as O
from test_fitsio_cpu import _NP, decode

CODES = {"D": 0, "E": 1, "J": 2, "K": 3, "I": 4, "B": 5}
FMT = {"D": ">f8", "E": ">f4", "J": ">i4", "K": ">i8", "I": ">i2", "B": "u1"}
_ROLE = {"t": "TIME", "f": "FLUX", "e": "FLUX_ERR", "q": "QUALITY", "c": "CADENCENO"}

_F64, _F32 = np.finfo(np.float64), np.finfo(np.float32)
SPECIALS = {
    "D": np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, np.nextafter(_F64.tiny, 0.0), _F64.tiny, _F64.max,
                   -_F64.max]),
    "E": np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, np.nextafter(_F32.tiny, np.float32(0)), _F32.tiny,
                   _F32.max, -_F32.max], dtype=np.float32),
}


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def real_values(letter, shape, rng):
    """Ordinary values with every class of SPECIALS[letter] among them (as many as fit), in the column's own precision."""
    n = int(np.prod(shape))
    v = (1e3 * rng.standard_normal(n)).astype(np.float32 if letter == "E" else np.float64)
    sp = SPECIALS[letter]
    at = rng.permutation(n)[:min(n, max(len(sp), n // 5))]
    v[at] = sp[np.arange(at.size) % len(sp)]
    return v.reshape(shape)


def fits_table(fields, n_rows, rng):
    """fields: (name, TFORM letter, repeat) in record order -> (rec, raw, offsets): a packed big-endian structured array of
    n_rows records, the same memory as uint8 [n_rows, row_bytes], and name -> byte offset.  Real columns hold real_values,
    integer and pad (`B` with a repeat) columns random bytes, so a field read at the wrong place reads noise."""
    dt = np.dtype([(name, FMT[letter]) if repeat == 1 else (name, FMT[letter], (repeat,)) for name, letter, repeat in fields])
    raw = rng.integers(0, 256, size=(n_rows, dt.itemsize), dtype=np.uint8)
    rec = raw.view(dt).reshape(n_rows)
    for name, letter, repeat in fields:
        if letter in "DE":
            rec[name] = real_values(letter, rec[name].shape, rng)
    return rec, raw, {name: dt.fields[name][1] for name in dt.names}


def write_fits(path, rec, tforms, telescop=None, cards=()):
    """A primary header and one BINTABLE holding `rec`: 80-character cards, 2880-byte blocks.  cards: extra (key, value)
    pairs for the extension header (TSCALn ...)."""
    def card(key, value):
        if isinstance(value, bool):
            text = "%20s" % ("T" if value else "F")
        elif isinstance(value, str):
            text = "'%-8s'" % value
        else:
            text = "%20s" % value
        return ("%-8s= %s" % (key, text)).ljust(80)

    def block(cards_):
        text = "".join(cards_) + "END".ljust(80)
        return text.ljust((len(text) + 2879) // 2880 * 2880).encode("ascii")

    primary = [card("SIMPLE", True), card("BITPIX", 8), card("NAXIS", 0), card("EXTEND", True)]
    if telescop:
        primary.append(card("TELESCOP", telescop))
    ext = [card("XTENSION", "BINTABLE"), card("BITPIX", 8), card("NAXIS", 2), card("NAXIS1", rec.dtype.itemsize),
           card("NAXIS2", rec.size), card("PCOUNT", 0), card("GCOUNT", 1), card("TFIELDS", len(tforms))]
    for i, (name, form) in enumerate(zip(rec.dtype.names, tforms), 1):
        ext += [card("TTYPE%d" % i, name), card("TFORM%d" % i, form)]
    ext += [card(k, v) for k, v in cards]
    data = rec.tobytes()
    with open(path, "wb") as fh:
        fh.write(block(primary) + block(ext) + data + b"\0" * (-len(data) % 2880))


def _col(raw, off, code, repeat=1):
    w = np.dtype(_NP[code]).itemsize * repeat
    return np.ascontiguousarray(raw[:, off:off + w]).view(_NP[code]).reshape(len(raw), repeat)


def decode_reference(raw, desc, bitmask, keep_nan_time=False, col=None, cube=None):
    """numpy restatement of the FITS decoders for one table -> dict.  Light-curve tables (lk_fits_unpack_batch): time, flux,
    flux_err, quality of the kept rows from `decode` (tests/test_fitsio_cpu.py), `keep` over all rows, and with col = (offset,
    code) the integer column `cadenceno` of the kept rows (lk_fits_cadenceno_batch).  cube = (column offsets, npix): the
    target-pixel rules of lk_fits_unpack_cube instead — rows kept by the quality flag alone when keep_nan_time, otherwise
    only with a finite time; a kept time that is not finite reads 0.0; `cubes` float32 [column, kept row, pixel]."""
    t = _col(raw, desc[2], desc[3]).ravel().astype(np.float64)
    q = _col(raw, desc[8], desc[9]).ravel().astype(np.int64) if desc[8] >= 0 else np.zeros(len(t), np.int64)
    flagged = (q & np.int64(bitmask)) != 0
    out = {}
    if cube is None:
        assert not keep_nan_time
        out["keep"] = keep = ~np.isnan(t) & ~flagged
        out["time"], out["flux"], out["flux_err"], out["quality"] = decode(types.SimpleNamespace(raw=raw), desc, bitmask)
        assert out["time"].size == int(keep.sum())
        if col is not None:
            out["cadenceno"] = _col(raw, col[0], col[1]).ravel().astype(np.int64)[keep]
    else:
        out["keep"] = keep = ~flagged & (np.isfinite(t) | bool(keep_nan_time))
        out["time"] = np.where(np.isfinite(t[keep]), t[keep], 0.0)
        out["quality"] = q[keep]
        offs, npix = cube
        out["cubes"] = np.stack([_col(raw, o, 1, npix).astype(np.float32)[keep] for o in offs])
    return out


# ------------------------------------------------------------------------------------------------ quality values
def quality_values(letter, bitmask, hit, rng):
    """One flag per row, in the column's type: rows with hit get a value with (sign-extended value & bitmask) != 0, the others
    one with no such bit that fits int32 (quality_out's type).  The pool holds the type's extremes, negative values, B values
    >= 128 and, for K, values with bits above 31 alone and together with low bits."""
    bits = {"J": 32, "K": 64, "I": 16, "B": 8}[letter]
    lo, hi = (0, 255) if letter == "B" else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    pool = [0, 1, 2, 4, 8, 16, 32, 64, 127, 128, 200, 254, 255, -1, -2, -128, -256, -4096, lo, hi, lo + 1, hi - 1]
    if letter == "K":
        pool += [1 << 32, 1 << 33, 1 << 40, (1 << 35) | 8, (1 << 62) | 0x20, -(1 << 40), (1 << 33) | 1, -(1 << 31), (1 << 31) - 1,
                 1 << 31, (1 << 40) | (1 << 33)]
    edge = np.array([v for v in pool if lo <= v <= hi], dtype=np.int64)
    rnd = rng.integers(max(lo, -(1 << 31)), min(hi, (1 << 31) - 1), size=512, endpoint=True)
    m = np.int64(bitmask)
    rnd = np.unique(np.concatenate([rnd, rnd & ~m, (rnd & ~m) | (m & -m)]))
    rnd = rnd[(rnd >= lo) & (rnd <= hi)]
    hit = np.asarray(hit, bool)

    def draw(pool):      # -> (a flagged value, an unflagged one) per row
        flagged = (pool & m) != 0
        yes, no = pool[flagged], pool[~flagged & (pool >= -(1 << 31)) & (pool < (1 << 31))]
        return [p[rng.integers(0, p.size, hit.size)] if p.size else None for p in (yes, no)]

    (e_yes, e_no), (r_yes, r_no) = draw(edge), draw(rnd)
    assert r_yes is not None and r_no is not None, (letter, bitmask)
    from_edge = rng.random(hit.size) < 0.5            # half the rows from the short list of edge values
    yes = r_yes if e_yes is None else np.where(from_edge, e_yes, r_yes)
    no = r_no if e_no is None else np.where(from_edge, e_no, r_no)
    return np.where(hit, yes, no)


# ------------------------------------------------------------------------------------------------ light-curve tables
def _fields(spec):
    fields, pads = [], 0
    for tok in spec.split():
        role, arg = tok.split(":")
        if role == "p":
            fields.append(("PAD%d" % pads, "B", int(arg)))
            pads += 1
        else:
            fields.append((_ROLE[role], arg, 1))
    return fields


# name -> (record layout, int64 bitmask, integer column of a table without CADENCENO: (role whose bytes are read, letter))
LAYOUTS = {
    # 12 bytes: the smallest record that holds D + E; no errors, no flags
    "d_e_12": ("t:D f:E", 0, ("f", "J")),
    # 13 bytes, every field at 1 mod 4; B flags >= 128 are unsigned: they never reach bit 40, odd ones hit bit 0
    "b_e_d_13": ("q:B t:E f:D", (1 << 40) | 1, ("q", "B")),
    "e_d_14": ("p:2 t:E f:D", 0, ("t", "J")),
    # I flags at an odd offset, B flags masked by their top bit
    "b_i_15": ("t:D f:E q:B c:I", 0x80, None),
    # E time at 1 mod 4, I flags at an odd offset, J cadence numbers at 3 mod 4
    "e_i_19": ("p:1 t:E q:I f:D c:J", 0x1C0, None),
    # TIME (D) at 4 mod 8, errors but no flags
    "e_d_d_20": ("f:E t:D e:D", 0, ("f", "J")),
    # J flags: a negative flag is sign-extended and hits bit 40
    "j_24": ("t:D f:E e:E q:J c:J", (1 << 40) | 0x15, None),
    # 27 bytes, fields at 2 mod 4, I flags: negative ones hit bit 40
    "i_27": ("p:2 t:D f:D e:E q:I c:B p:2", (1 << 40) | 0x28, None),
    # aligned K flags and K cadence numbers under a small mask: negative flags with clear low bits are kept
    "k_40": ("t:D f:D e:D q:K c:K", 0xA8, None),
    # 100 bytes, fields at 3 mod 4, K flags with bits above 31
    "k_100": ("p:3 t:E f:E e:E q:K c:J p:73", (1 << 40) | (1 << 33) | 0xA8, None),
    # 511 bytes, the decoded fields behind 470 bytes of padding, K cadence numbers at 2 mod 4
    "j_511": ("t:D p:470 f:E e:D q:J c:K p:9", 0xA8, None),
    # 512 bytes (the LDS stage's limit), fields at 1 mod 4, the last field ends the record; a negative bitmask
    "i_512": ("p:1 t:D f:D e:D q:I p:483 c:I", -256, None),
}
ROWS = (0, 1, 255, 256, 257, 513, 1300)
# (layout, rows, keep pattern): all kept, none kept (by flags, by NaN times), only the last row of the last trip kept
DESIGNATED = (("j_511", 513, "all"), ("d_e_12", 1300, "all"), ("i_27", 257, "none"), ("e_d_14", 256, "none"),
              ("k_100", 1300, "last"), ("i_512", 257, "last"))
SHARE_MIN_ROWS = 255   # a table of 0 or 1 rows has no share between 25 % and 75 %


def make_table(layout, n_rows, keep="share", seed=0, bitmask=None):
    """One table of LAYOUTS[layout].  keep: 'share' (flags hit ~45 % of the rows, ~8 % of the times are NaN; without a flag
    column ~45 % of the times are NaN), 'all', 'none', 'last'.  bitmask: instead of the layout's own."""
    spec, own_mask, alias = LAYOUTS[layout]
    bitmask = own_mask if bitmask is None else bitmask
    fields = _fields(spec)
    rng = np.random.default_rng(_seed(layout, n_rows, keep, seed))
    rec, raw, offs = fits_table(fields, n_rows, rng)
    letters = {name: letter for name, letter, _ in fields}
    has_q = "QUALITY" in offs
    if keep == "share":
        nan_t, hit = rng.random(n_rows) < (0.08 if has_q else 0.45), rng.random(n_rows) < 0.45
    elif keep == "all":
        nan_t, hit = np.zeros(n_rows, bool), np.zeros(n_rows, bool)
    else:
        hit = np.ones(n_rows, bool)
        nan_t = rng.random(n_rows) < 0.5 if has_q else hit.copy()
        if keep == "last":
            hit[-1] = nan_t[-1] = False
    t = rec["TIME"]
    t[np.isnan(t)] = 1.5
    t[nan_t] = np.nan
    if has_q:
        rec["QUALITY"] = quality_values(letters["QUALITY"], bitmask, hit, rng)
    if "CADENCENO" in offs:
        info = np.iinfo(np.int32 if letters["CADENCENO"] in "JK" else rec["CADENCENO"].dtype.newbyteorder("="))
        rec["CADENCENO"] = rng.integers(info.min, info.max, size=n_rows, endpoint=True)
        col = (offs["CADENCENO"], CODES[letters["CADENCENO"]])
    else:
        col = (offs[_ROLE[alias[0]]], CODES[alias[1]])

    def field(name):
        return (offs[name], CODES[letters[name]]) if name in offs else (-1, 0)

    desc = np.array((rec.dtype.itemsize, n_rows) + field("TIME") + field("FLUX") + field("FLUX_ERR") + field("QUALITY"),
                    dtype=np.int32)
    tforms = ["%d%s" % (rep, letter) for _, letter, rep in fields]
    return types.SimpleNamespace(name="%s-%d-%s" % (layout, n_rows, keep), layout=layout, keep=keep, rec=rec, raw=raw, desc=desc,
                                 bitmask=bitmask, col=col, tforms=tforms, offsets=offs, letters=letters)


@functools.lru_cache(maxsize=None)
def layout_tables():
    """Every layout at every row count, then the designated keep patterns: ONE ragged batch, so the 512-byte records size the
    LDS stage for the 12-byte tables too."""
    tabs = [make_table(name, n) for n in ROWS for name in LAYOUTS]
    return tuple(tabs + [make_table(name, n, keep) for name, n, keep in DESIGNATED])


@functools.lru_cache(maxsize=None)
def small_tables(B):
    """B tables of 3 rows x 12 bytes (B > 1024: the offset scan gives every thread more than one count)."""
    big = make_table("d_e_12", 3 * B, seed=B)
    out = []
    for b in range(B):
        desc = big.desc.copy()
        desc[1] = 3
        out.append(types.SimpleNamespace(name="small-%d" % b, layout="d_e_12", keep="share", raw=big.raw[3 * b:3 * b + 3], desc=desc,
                                         bitmask=0, col=big.col))
    return tuple(out)


def batch_reference(tables):
    """What lk_fits_unpack_batch + lk_fits_cadenceno_batch return for `tables`: dict of concatenated columns and new_off."""
    refs = [decode_reference(t.raw, t.desc, t.bitmask, col=t.col) for t in tables]
    out = {k: np.concatenate([r[k] for r in refs]) for k in ("time", "flux", "flux_err", "quality", "cadenceno")}
    out["new_off"] = np.concatenate([[0], np.cumsum([r["time"].size for r in refs])]).astype(np.int64)
    out["kept"] = np.array([r["keep"].mean() if r["keep"].size else np.nan for r in refs])
    return out


# ------------------------------------------------------------------------------------------------ pixel cubes
# name -> (npix, ncols, rows, TIME letter, QUALITY letter, bytes before TIME, bytes after the last column, bitmask)
# row_bytes mod 4 decides how the aligned and the byte-wise branch of the cube kernel alternate from row to row
# bitmask -1: every row flagged; the one-row tables are not flagged (ONE_ROW has their time and pixel)
ONE_ROW = {"p1_c1_r1": (1234.5678, -3.25e-3), "p1_c1_r1_nan_time": (np.nan, 7.0e10)}
CUBES = {
    "p1_c1_r1": (1, 1, 1, "D", "J", 0, 0, 0x15),                 # 16-byte records, one pixel, kept
    "p1_c1_r1_nan_time": (1, 1, 1, "D", "I", 1, 0, 0x15),        # 15-byte records; kept only under keep_nan_time, time reads 0
    "p127_c2_r255_mod1": (127, 2, 255, "D", "I", 3, 0, 0x15),     # 3 + 8 + 2 + 1016 = 1029
    "p128_c3_r256_mod2": (128, 3, 256, "E", "J", 0, 2, 0x15),     # 4 + 4 + 1536 + 2 = 1546
    "p129_c4_r257_mod3": (129, 4, 257, "D", "I", 1, 0, 0x15),     # 1 + 8 + 2 + 2064 = 2075
    "p400_c3_r600_mod1": (400, 3, 600, "D", "J", 0, 1, 0x15),     # an FFI cut-out: four trips of the 128-pixel loop
    "p400_c1_r600_mod0_skewed": (400, 1, 600, "D", "J", 1, 3, 0x15),   # rows aligned, the column at 1 mod 4: byte-wise always
    "p128_c4_r600_mod2": (128, 4, 600, "D", "I", 0, 0, 0x15),     # 8 + 2 + 2048 = 2058
    "p129_c2_r257_none_kept": (129, 2, 257, "D", "J", 0, 0, -1),
}


@functools.lru_cache(maxsize=None)
def cube_table(name):
    npix, ncols, n_rows, lt, lq, lead, tail, bitmask = CUBES[name]
    fields = ([("PAD0", "B", lead)] if lead else []) + [("TIME", lt, 1), ("QUALITY", lq, 1)]
    fields += [("PIX%d" % c, "E", npix) for c in range(ncols)] + ([("PAD1", "B", tail)] if tail else [])
    rng = np.random.default_rng(_seed("cube", name))
    rec, raw, offs = fits_table(fields, n_rows, rng)
    # real_values put NaN and +-inf among the times (a third of them at least when there are few rows)
    if bitmask == -1:
        rec["QUALITY"] = quality_values(lq, bitmask, np.ones(n_rows, bool), rng)
        rec["QUALITY"][rec["QUALITY"] == 0] = 1
    elif name in ONE_ROW:
        rec["QUALITY"] = quality_values(lq, bitmask, np.zeros(n_rows, bool), rng)
        rec["TIME"], rec["PIX0"] = ONE_ROW[name]
    else:
        rec["QUALITY"] = quality_values(lq, bitmask, rng.random(n_rows) < 0.4, rng)
    return types.SimpleNamespace(name=name, rec=rec, raw=raw, npix=npix, bitmask=bitmask, off_time=offs["TIME"], code_time=CODES[lt],
                                 off_quality=offs["QUALITY"], code_quality=CODES[lq],
                                 col_offsets=[offs["PIX%d" % c] for c in range(ncols)],
                                 desc=np.array([rec.dtype.itemsize, n_rows, offs["TIME"], CODES[lt], offs["TIME"], CODES[lt], -1, 0,
                                                offs["QUALITY"], CODES[lq]], dtype=np.int32),
                                 tforms=["%d%s" % (rep, letter) for _, letter, rep in fields])


def cube_reference(c, keep_nan_time):
    return decode_reference(c.raw, c.desc, c.bitmask, keep_nan_time=keep_nan_time, cube=(c.col_offsets, c.npix))


# ------------------------------------------------------------------------------------------------ remove_nans compaction
COMPACT_N = (0, 1, 63, 64, 65, 511, 512, 513, 1025, 4097)
COMPACT_PATTERNS = ("none", "all", "alternating", "first_half", "last_half", "every_64th_kept", "strip")


def nan_pattern(pattern, n):
    i = np.arange(n)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "first_half":
        return i < n // 2
    if pattern == "last_half":
        return i >= n // 2
    if pattern == "every_64th_kept":
        return i % 64 != 17
    # the pack kernel gives each of its 8 waves a strip of ceil(n / 8) cadences rounded up to 64: the second wave's whole strip
    # is NaN (the first wave's when there is no second)
    strip = ((n + 7) // 8 + 63) // 64 * 64
    lo = strip if n > strip else 0
    return (i >= lo) & (i < lo + strip)


@functools.lru_cache(maxsize=None)
def compaction_cases():
    """-> (names, time, flux, flux_err, n_off): one ragged batch, size-major with one empty target (n = 0) after each of the
    first sizes, so the empty targets and the all-NaN ones sit between ordinary targets."""
    rng = np.random.default_rng(20)
    names, fs = [], []

    def add(pattern, n):
        f = 1000.0 + 100.0 * rng.standard_normal(n)
        f[nan_pattern(pattern, n)] = np.nan
        names.append("%s-%d" % (pattern, n))
        fs.append(f)

    for g, n in enumerate(n for n in COMPACT_N if n):
        for pattern in COMPACT_PATTERNS:
            add(pattern, n)
        if g < len(COMPACT_PATTERNS):
            add(COMPACT_PATTERNS[g], 0)
    flux = np.concatenate(fs)
    n_off = np.concatenate([[0], np.cumsum([f.size for f in fs])]).astype(np.int64)
    time = np.cumsum(rng.random(flux.size))
    err = rng.random(flux.size) + 0.5
    err[rng.random(flux.size) < 0.05] = np.nan
    return names, time, flux, err, n_off


# ------------------------------------------------------------------------------------------------ transit masks
@functools.lru_cache(maxsize=None)
def mask_cases():
    """-> dict: one ragged call (time, n_off, period / duration / transit_time over all planets, p_off) and the targets' names.
    The 1000-cadence target sets the grid; every other target ends inside its first or second 256-cadence tile."""
    rng = np.random.default_rng(21)
    bjd = 2.4e6 + np.sort(rng.uniform(0.0, 30.0, 256))
    bjd[[3, 77]] = np.nan
    bjd[[0, 255]] = -np.inf, np.inf
    dyadic = (4.0, 0.5, 1.0)
    # five planets that each mark cadences no other marks (the CPU test takes them out one by one); a planet that marks
    # everything (duration >= period) or nothing (duration 0) would hide the others: those have targets of their own
    dyadic5 = [(4.0, 0.5, 101.0), (-4.0, 0.5, 103.0), (8.0, 1.0, 100.5), (16.0, 0.25, 6.0), (-2.0, 0.125, 0.5)]
    bjd5 = [(0.3, 0.05, 2.4e6 + 0.1), (-2.1, 0.4, 2.4e6 + 5.0), (3.7, 0.2, 2.4e6 - 11.0), (1.1, 0.1, 2.4e6 + 0.45),
            (-0.7, 0.05, 2.4e6 + 0.33)]
    targets = [
        ("dyadic_255_1p", np.arange(255) / 64.0, [dyadic]),
        ("empty_5p", np.zeros(0), dyadic5),
        ("zero_planets_257", np.sort(rng.uniform(0.0, 30.0, 257)), []),
        ("one_on_the_boundary_1p", np.array([1.25]), [dyadic]),
        # full BJD: t / P ~ 1e7 for P = 0.3, negative periods, NaN and +-inf times
        ("bjd_256_5p", bjd, bjd5),
        ("dyadic_1000_1p", np.arange(1000) / 64.0, [dyadic]),
        ("empty_0p", np.zeros(0), []),
        ("dyadic_257_5p", 100.0 + np.arange(257) / 64.0, dyadic5),
        ("negative_period_256_1p", np.sort(rng.uniform(-7.0, 9.0, 256)), [(-2.1, 0.4, 5.0)]),
        ("bjd_p03_alone_256_1p", bjd, [bjd5[0]]),
        ("duration_ge_period_256_1p", bjd, [(1.5, 2.0, 2.4e6)]),                     # every time that is a number
        ("duration_zero_255_1p", np.arange(255) / 64.0, [(2.0, 0.0, 1.0)]),             # nothing, the cadences at phase 0 included
    ]
    planets = [p for _, _, ps in targets for p in ps]
    return dict(names=[n for n, _, _ in targets], time=np.concatenate([t for _, t, _ in targets]),
                n_off=np.concatenate([[0], np.cumsum([t.size for _, t, _ in targets])]).astype(np.int64),
                p_off=np.concatenate([[0], np.cumsum([len(ps) for _, _, ps in targets])]).astype(np.int32),
                period=np.array([p[0] for p in planets]), duration=np.array([p[1] for p in planets]),
                transit_time=np.array([p[2] for p in planets]))


def mask_reference(m, b):
    """O.transit_mask for target b of mask_cases()."""
    t = m["time"][m["n_off"][b]:m["n_off"][b + 1]]
    s = slice(m["p_off"][b], m["p_off"][b + 1])
    with np.errstate(invalid="ignore"):
        return O.transit_mask(t, m["period"][s], m["duration"][s], m["transit_time"][s])


def dyadic_boundary(k, k0=64, period=256, half_width=16):
    """For times k / 64 d, period 4 d, duration 0.5 d, transit time 1 d, in integers: (cadences with |phase| == 0.25 d
    exactly, cadences with |phase| < 0.25 d)."""
    d = (np.asarray(k) - k0) % period
    d = np.minimum(d, period - d)
    return d == half_width, d < half_width


# ------------------------------------------------------------------------------------------------ bin
BIN_SIZE = 0.25       # d: 16 cadences of 1/64 d, 21600 s


@functools.lru_cache(maxsize=None)
def bin_cases():
    """-> dict name -> call: dict(time, flux, flux_err (or None), n_off, names, start (None, a scalar or one per target)).
    Every time is a multiple of 1/64 d except in the 'random' targets, so with 0.25 d bins the edge membership is exact."""
    rng = np.random.default_rng(22)

    def good(n):
        return 0.5 + rng.random(n)

    k_gap = np.concatenate([np.arange(101), 6400 + np.arange(60)])           # 100 d without a cadence: 400 empty bins
    k_dup = np.repeat(np.arange(0, 130, 2), 3)
    e_part = good(k_dup.size)
    e_part[::4], e_part[5::16] = np.nan, np.inf
    e_part[48:96] = np.nan                                                    # a whole bin without a finite error
    f_dup = rng.standard_normal(k_dup.size)
    f_dup[::5] = np.nan
    f_hole = rng.standard_normal(193)
    f_hole[33:49] = np.nan                                                    # bin (0.5 d, 0.75 d]: no flux at all
    t_rand = np.sort(rng.uniform(2.0, 9.0, 700))
    e_rand = good(700)
    e_rand[10] = np.inf
    nan = np.full
    general = [
        ("span_3d", np.arange(193) / 64.0, rng.standard_normal(193), good(193)),      # 12 bins, the last cadence on the last edge
        ("empty", np.zeros(0), np.zeros(0), np.zeros(0)),
        ("duplicates_partial_err", k_dup / 64.0, f_dup, e_part),
        ("one_cadence", np.array([0.5]), np.array([2.0]), np.array([1.0])),               # zero bins
        ("gap_nan_err", k_gap / 64.0, rng.standard_normal(k_gap.size), nan(k_gap.size, np.nan)),
        ("one_time_five_cadences", np.full(5, 1.5), rng.standard_normal(5), good(5)),     # zero bins
        ("nan_flux_bin_no_err", np.arange(193) / 64.0, f_hole, nan(193, np.nan)),
        ("late_start", 2.0 + np.arange(100) / 64.0, rng.standard_normal(100), good(100)),
        ("random", t_rand, rng.standard_normal(700), e_rand),
    ]
    ints = []
    for name, k in (("int_span_3d", np.arange(193)), ("int_gap", k_gap), ("int_duplicates", k_dup), ("int_one", np.array([7])),
                    ("int_long", np.arange(0, 5000, 3))):
        f = rng.integers(-(1 << 20), 1 << 20, size=k.size, endpoint=True).astype(np.float64)
        f[rng.random(k.size) < 0.1] = np.nan
        if name == "int_span_3d":
            f[16:33] = np.nan                                                 # cadence 16 is bin 0's, so bin 1 = (16, 32] is all NaN
        ints.append((name, k / 64.0, f, np.full(k.size, 2.0)))

    def call(targets, start=None, err=True):
        return dict(names=[t[0] for t in targets], time=np.concatenate([t[1] for t in targets]),
                    flux=np.concatenate([t[2] for t in targets]), flux_err=np.concatenate([t[3] for t in targets]) if err else None,
                    n_off=np.concatenate([[0], np.cumsum([t[1].size for t in targets])]).astype(np.int64), start=start)

    per_target = np.array([-0.125, 0.0, 0.5, 0.5, 1.0, 1.5, 0.0, 2.25, 100.0])   # before / on / after the first cadence, past the last
    return {
        "general": call(general),
        "start_before": call(general, start=-0.125),
        "start_after": call(general, start=1.0),
        "start_per_target": call(general, start=per_target),
        "no_err_array": call(general, err=False),
        "integers": call(ints),
        "integers_start_after": call(ints, start=0.75),
    }


def bin_reference(c, b):
    """O.bin_lightcurve for target b of a call of bin_cases() -> (time, flux, flux_err); no bins for an empty target and for
    one whose last cadence is not after the start."""
    s = slice(c["n_off"][b], c["n_off"][b + 1])
    t, f = c["time"][s], c["flux"][s]
    e = c["flux_err"][s] if c["flux_err"] is not None else np.full(t.size, np.nan)
    start = None if c["start"] is None else float(np.broadcast_to(c["start"], (len(c["names"]),))[b])
    if t.size == 0 or not (t[-1] - (t[0] if start is None else start)) > 0:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    return O.bin_lightcurve(t, f, e, BIN_SIZE, time_bin_start=start)
