"""GPU: phase-binned folded light curves on the resident batch against the numpy restatement of tests/foldbin_cases.py.

``DeviceFoldedBatch.cycle / odd_mask / even_mask / bin`` and the fused ``DeviceLightCurveBatch.fold_bin`` on one batch of light
curves with 5000, 1, 63, 0, 64, 65 and 1500 cadences (empty, single cadence, the wave boundary, more than one pass of a
1024-thread workgroup and FOLD_TILE = 4096 crossed) whose periods give about 20 cycles, exactly one cycle, a period
commensurate with the cadence (whole bins empty) and times on binary fractions with phases exactly on bin edges; NaN flux
scattered, one bin all NaN, one light curve without a finite error beside ones with errors, and a batch without flux_err.

Tolerances: the bin layout, the counts, the NaN pattern and the bin centres are exact; flux and flux_err agree within the
project's 1e-9 relative (README, "Parity statements"); the median is bitwise ``np.nanmedian``.  Every comparison prints its
largest relative difference before it asserts (``pytest -s``); DESIGN.md 4.2d records the largest ones measured."""
import functools

import numpy as np
import pytest

import foldbin_cases as C
from lightkurve_amd import _capi, batch as lkbatch, foldbin
from lightkurve_amd.device import DeviceLightCurveBatch, DevicePhaseCurveBatch
from lightkurve_amd.lightcurve import LightCurve

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ALL = tuple(range(len(C.LENGTHS)))
TWO_PLUS = tuple(b for b, n in enumerate(C.LENGTHS) if n >= 2)      # bins= needs two cadences
NO_ERR = (5, 6, 4)                                                   # the batch without flux_err


def _pack(idx, with_err=True):
    tg = [C.batch()[b] for b in idx]
    n_off = np.concatenate([[0], np.cumsum([t["time"].size for t in tg])]).astype(np.int64)
    cat = lambda k: np.concatenate([t[k] for t in tg]) if tg else np.zeros(0)
    return cat("time"), cat("flux"), (cat("flux_err") if with_err else None), n_off, np.array([t["period"] for t in tg])


@functools.lru_cache(maxsize=None)
def dev(idx=ALL, with_err=True):
    time, flux, err, n_off, period = _pack(idx, with_err)
    return DeviceLightCurveBatch.from_arrays(time, flux, err, n_off), period


@functools.lru_cache(maxsize=None)
def dev_folded(idx=ALL, with_err=True, epoch_given=False):
    b, period = dev(idx, with_err)
    epoch = np.array([C.batch()[i]["time"][0] if C.LENGTHS[i] else 0.0 for i in idx]) if epoch_given else None
    return b.fold(period, epoch_time=epoch)


FORMS = {
    "size": dict(time_bin_size=0.01),
    "size_nbins": dict(time_bin_size=0.02, n_bins=30),
    "per_target": None,           # filled per batch: arrays of sizes and starts
    "bins": dict(bins=25),
}


def form_kwargs(form, idx):
    if form == "per_target":
        sizes, starts = C.per_target_sizes()
        return dict(time_bin_size=sizes[list(idx)], time_bin_start=starts[list(idx)])
    return dict(FORMS[form])


def reference(idx, form, which="all", aggregate="mean", with_err=True, epoch_given=False, **extra):
    """The restatement for every light curve of the batch -> dict of concatenated arrays + bin_off."""
    fo = C.folded(epoch_given, with_err)
    kw = form_kwargs(form, idx) if form else {}
    kw.update(extra)
    parts = []
    for j, b in enumerate(idx):
        f = fo[b]
        size = kw.get("time_bin_size")
        size = None if size is None else float(np.broadcast_to(size, (len(idx),))[j])
        start = kw.get("time_bin_start")
        start = None if start is None else float(np.broadcast_to(start, (len(idx),))[j])
        parts.append(C.phase_bin_reference(f["phase"], f["flux"], f["flux_err"], f["cycle"], size=size, start=start,
                                           n_bins=kw.get("n_bins"), bins=kw.get("bins"), aggregate=aggregate, which=which))
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("phase", "flux", "flux_err", "count")}
    out["bin_off"] = np.concatenate([[0], np.cumsum([p["phase"].size for p in parts])]).astype(np.int64)
    return out


def max_rel(a, b):
    m = ~np.isnan(b) & (b != 0)
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def assert_same(got, ref, label, exact_flux=False):
    assert np.array_equal(got["bin_off"], ref["bin_off"]), label
    assert np.array_equal(got["count"], ref["count"]), label
    assert np.array_equal(got["phase"], ref["phase"]), label                         # bin centres: bitwise
    for k in ("flux", "flux_err"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (label, k)
    print("%s: max rel diff flux %.3g, flux_err %.3g" % (label, max_rel(got["flux"], ref["flux"]),
                                                         max_rel(got["flux_err"], ref["flux_err"])))
    if exact_flux:
        assert np.array_equal(got["flux"], ref["flux"], equal_nan=True), label
    else:
        np.testing.assert_allclose(got["flux"], ref["flux"], rtol=RTOL, atol=0, err_msg=str(label))
    np.testing.assert_allclose(got["flux_err"], ref["flux_err"], rtol=RTOL, atol=0, err_msg=str(label))


# ------------------------------------------------------------------------------------------------ 1. cycle / odd / even
@pytest.mark.parametrize("epoch_given", [False, True])
def test_cycle_and_masks(epoch_given):
    fd = dev_folded(ALL, True, epoch_given)
    fo = C.folded(epoch_given)
    cyc = np.concatenate([f["cycle"] for f in fo])
    assert np.array_equal(fd.to_host()["phase"], np.concatenate([f["phase"] for f in fo]))
    got = fd.cycle()
    assert got.dtype == np.int64 and np.array_equal(got, cyc)
    odd, even = fd.odd_mask(), fd.even_mask()
    assert odd.dtype == bool and np.array_equal(odd, cyc % 2 == 1) and np.array_equal(even, cyc % 2 == 0)
    assert cyc.max() >= 19 and odd.any() and even.any()
    # device masks into select: the same light curves as the host masks
    lcs = fd.as_lightcurves()
    for dm, hm in ((fd.odd_mask(to_host=False), odd), (fd.even_mask(to_host=False), even)):
        a, b = lcs.select(dm), lcs.select(hm)
        assert np.array_equal(a.n_off, b.n_off) and a.n_off[-1] == hm.sum()
        assert np.array_equal(a.time_host(), b.time_host()) and np.array_equal(a.flux_host(), b.flux_host(), equal_nan=True)
        assert np.array_equal(a.time_host(), np.concatenate([f["phase"] for f in fo])[hm])


# ------------------------------------------------------------------------------------------------ 2. fold().bin()
@pytest.mark.parametrize("aggregate", ["mean", "median"])
@pytest.mark.parametrize("which", ["all", "odd", "even"])
@pytest.mark.parametrize("form", ["size", "size_nbins", "per_target", "bins"])
def test_fold_then_bin(form, which, aggregate):
    idx = TWO_PLUS if form == "bins" else ALL
    res = dev_folded(idx).bin(aggregate_func=aggregate, which=which, **form_kwargs(form, idx))
    assert isinstance(res, DevicePhaseCurveBatch) and len(res) == len(idx)
    ref = reference(idx, form, which, aggregate)
    assert ref["count"].sum() > 0 and (ref["count"] == 0).any() and np.isnan(ref["flux"][ref["count"] > 0]).any()
    assert_same(res.to_host(), ref, (form, which, aggregate), exact_flux=aggregate == "median")


def test_fold_then_bin_default_size_and_phases_on_edges():
    # default time_bin_size = 0.5 as in the reference
    assert_same(dev_folded(ALL).bin().to_host(), reference(ALL, None), "default")
    # the light curve on binary fractions, size 1/8 from -1/2: phases (multiples of 1/16) on every edge go to the lower bin,
    # the one at -1/2 (r == 0) to bin 0
    ref = reference((C.EXACT,), "per_target")
    assert ref["count"].tolist() == [12, 8, 8, 8, 8, 8, 8, 4]
    assert_same(dev_folded((C.EXACT,)).bin(time_bin_size=0.125, time_bin_start=-0.5).to_host(), ref, "exact")
    # from the default start -1/2 the last slot (phase 7/16) has r = 15/16 d; with size 15/64 d that is exactly the last of
    # ceil(4.0) = 4 edges (20250 s steps, all exact), and membership needs r < edges[n_bins]: the four slots there are dropped
    ref = reference((C.EXACT,), None, time_bin_size=15.0 / 64.0)
    assert ref["count"].sum() == 60 and ref["bin_off"][-1] == 4
    assert_same(dev_folded((C.EXACT,)).bin(time_bin_size=15.0 / 64.0).to_host(), ref, "last edge")


@pytest.mark.parametrize("aggregate", ["mean", "median"])
def test_batch_without_flux_err(aggregate):
    fd = dev_folded(NO_ERR, False)
    assert fd.d_flux_err is None
    ref = reference(NO_ERR, "size", "all", aggregate, with_err=False)
    assert_same(fd.bin(time_bin_size=0.01, aggregate_func=aggregate).to_host(), ref, ("no err", aggregate), aggregate == "median")
    b, period = dev(NO_ERR, False)
    assert_same(b.fold_bin(period, time_bin_size=0.01, which="odd").to_host(), reference(NO_ERR, "size", "odd", with_err=False),
                "no err fused")


def test_argument_errors_on_the_device_objects():
    fd = dev_folded(ALL)
    b, period = dev(ALL)
    with pytest.raises(ValueError):
        fd.bin(bins=25)                       # light curves with 0 and 1 cadences: i < 2
    with pytest.raises(ValueError):
        b.fold_bin(period, bins=25)
    with pytest.raises(ValueError):
        fd.bin(bins=25, time_bin_size=0.1)
    with pytest.raises(ValueError):
        fd.bin(bins=25, n_bins=3)
    with pytest.raises(ValueError):
        fd.bin(aggregate_func="sum")
    with pytest.raises(ValueError):
        fd.bin(which="both")
    with pytest.raises(ValueError, match=r"fold\(\.\.\.\)\.bin"):
        b.fold_bin(period, aggregate_func="median")


# ------------------------------------------------------------------------------------------------ 3. fused fold_bin
@pytest.mark.parametrize("which", ["all", "odd", "even"])
@pytest.mark.parametrize("form", ["size", "size_nbins", "per_target", "bins"])
def test_fused_matches_fold_then_bin(form, which):
    idx = TWO_PLUS if form == "bins" else ALL
    b, period = dev(idx)
    kw = form_kwargs(form, idx)
    fused = b.fold_bin(period, which=which, **kw).to_host()
    assert_same(fused, dev_folded(idx).bin(which=which, **kw).to_host(), ("fused vs fold().bin()", form, which))
    assert_same(fused, reference(idx, form, which), ("fused vs numpy", form, which))


def test_fused_with_epoch_given():
    b, period = dev(ALL)
    epoch = np.array([C.batch()[i]["time"][0] if C.LENGTHS[i] else 0.0 for i in ALL])
    for which in ("odd", "even"):
        fused = b.fold_bin(period, epoch_time=epoch, time_bin_size=0.01, which=which).to_host()
        assert_same(fused, reference(ALL, "size", which, epoch_given=True), ("epoch given", which))
        assert_same(fused, dev_folded(ALL, True, True).bin(time_bin_size=0.01, which=which).to_host(), ("epoch given, two routes", which))


# ------------------------------------------------------------------------------------------------ 4. the LDS limit
@pytest.mark.parametrize("n_bins", [foldbin.LDS_BINS, foldbin.LDS_BINS + 1])
def test_bins_at_the_lds_limit(n_bins):
    """1024 bins per target are accumulated in LDS, 1025 in the slab of device memory: both give fold().bin()'s result."""
    assert foldbin.LDS_BINS == 1024
    b, period = dev(ALL)
    kw = dict(time_bin_size=0.004, n_bins=n_bins)
    fused = b.fold_bin(period, **kw).to_host()
    nb = np.diff(fused["bin_off"])
    assert nb.tolist() == [n_bins if n else 0 for n in C.LENGTHS]
    assert_same(fused, dev_folded(ALL).bin(**kw).to_host(), ("limit, two routes", n_bins))
    assert_same(fused, reference(ALL, None, **kw), ("limit vs numpy", n_bins))
    odd = b.fold_bin(period, which="odd", **kw).to_host()
    assert_same(odd, reference(ALL, None, which="odd", **kw), ("limit odd", n_bins))


# ------------------------------------------------------------------------------------------------ 5. determinism
def _bitwise(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("phase", "flux", "flux_err", "count", "bin_off"))


@pytest.mark.parametrize("kw", [dict(time_bin_size=0.01), dict(time_bin_size=0.004, n_bins=foldbin.LDS_BINS + 1)], ids=["lds", "slab"])
def test_fused_is_reproducible_and_independent_of_the_batch(kw):
    b, period = dev(ALL)
    first = b.fold_bin(period, which="even", **kw).to_host()
    assert _bitwise(first, b.fold_bin(period, which="even", **kw).to_host())
    # every light curve alone
    for j in (0, C.NANSTD, C.COMMENSURATE):
        one, p1 = dev((j,))
        alone = one.fold_bin(p1, which="even", **kw).to_host()
        lo, hi = first["bin_off"][j], first["bin_off"][j + 1]
        for k in ("phase", "flux", "flux_err", "count"):
            assert np.array_equal(alone[k], first[k][lo:hi], equal_nan=True), (j, k)
    # the light curves in reversed order
    rev_idx = ALL[::-1]
    rb, rp = dev(rev_idx)
    rev = rb.fold_bin(rp, which="even", **kw).to_host()
    for j, b0 in enumerate(rev_idx):
        lo, hi = first["bin_off"][b0], first["bin_off"][b0 + 1]
        rlo, rhi = rev["bin_off"][j], rev["bin_off"][j + 1]
        for k in ("phase", "flux", "flux_err", "count"):
            assert np.array_equal(rev[k][rlo:rhi], first[k][lo:hi], equal_nan=True), (b0, k)


# ------------------------------------------------------------------------------------------------ 6. host pointers
def test_host_pointer_forms_equal_the_resident_form():
    b, period = dev(ALL)
    time, flux, err, n_off, _ = _pack(ALL)
    for kw in (dict(time_bin_size=0.01, which="odd"), dict(time_bin_size=0.004, n_bins=foldbin.LDS_BINS + 1)):
        want = b.fold_bin(period, **kw).to_host()
        assert _bitwise(_capi.fold_bin_batch(time, flux, n_off, period, flux_err=err, **kw), want)
    lcs = [LightCurve(time=t["time"], flux=t["flux"], flux_err=t["flux_err"]) for t in C.batch()]
    assert _bitwise(lkbatch.fold_bin_batch(lcs, period, time_bin_size=0.01, which="odd"),
                    b.fold_bin(period, time_bin_size=0.01, which="odd").to_host())
    b2, p2 = dev(TWO_PLUS)
    t2, f2, e2, o2, _ = _pack(TWO_PLUS)
    assert _bitwise(_capi.fold_bin_batch(t2, f2, o2, p2, flux_err=e2, bins=25), b2.fold_bin(p2, bins=25).to_host())


# ------------------------------------------------------------------------------------------------ 7. after a box search
def test_bls_fold_bin_puts_the_transit_at_phase_zero():
    rng = np.random.RandomState(5)
    lcs, true_p = [], (2.0, 2.3, 1.7)
    for P in true_p:
        t = 100.0 + 0.03 * np.arange(400)
        f = 1.0 + 1e-4 * rng.randn(t.size)
        f[np.abs((t - 100.7 + 0.5 * P) % P - 0.5 * P) < 0.1] -= 0.01          # duration 0.2 d, depth 1 %
        lcs.append(LightCurve(time=t, flux=f, flux_err=np.full(t.size, 1e-4)))
    res = DeviceLightCurveBatch.from_lightcurves(lcs).bls(np.linspace(1.6, 2.4, 81), duration=[0.2])
    pk = res.peaks()
    assert np.allclose(pk["period"], true_p, atol=0.011)
    pc = res.fold_bin(bins=15).to_host()
    two = res.fold().bin(bins=15).to_host()
    assert np.array_equal(pc["bin_off"], two["bin_off"]) and np.array_equal(pc["count"], two["count"])
    np.testing.assert_allclose(pc["flux"], two["flux"], rtol=RTOL, atol=0)
    for b in range(3):
        lo, hi = pc["bin_off"][b], pc["bin_off"][b + 1]
        centre, flux = pc["phase"][lo:hi], pc["flux"][lo:hi]
        half = 0.5 * (centre[1] - centre[0])
        k = int(np.nanargmin(flux))
        assert centre[k] - half <= 0.0 <= centre[k] + half, (b, centre[k], half)
        assert flux[k] < 0.995
