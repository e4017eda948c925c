"""GPU: the shared-design-matrix regression for RAGGED batches aligned by cadence (lk_regress_shared_rows_batch*,
lk_align_rows_batch*, lk_ridge_prior_rows_*_batch*, lk_fits_cadenceno_batch*; DeviceLightCurveBatch.regression_correct(rows= /
cadenceno=), .cbv_correct(cadenceno=), .d_cadenceno) against the numpy oracle per target on X[rows_b].  Inputs and the oracle's
answers come from regress_rows_cases.py, which asserts on the reference side that no residual of any clip pass is within 1e-3
standard deviations of a clip bound (the four configurations have 0.014 .. 0.068), so a kernel right to 1e-9 cannot flip a
mask.  Tolerances are the house ones of test_regress_shared_gpu.py: outlier masks identical, model within 1e-9 std(y_b),
coefficients rtol 1e-6 / atol 1e-9.

Grid padding (test_a_target_alone_in_the_batch_and_on_a_padded_grid): the order of a target's partial sums is a function of
the grid's row count (shared_split(Nx)), so bytes are compared where the slices keep their bounds (21 rows appended to 1003:
four slices of 256 either way) and the 100 appended rows of the issue, which move the slice bounds (five slices of 224), are
compared through what does not depend on Nx: identical outlier masks and the house tolerances on model and coefficients."""
import os

import numpy as np
import pytest

from lightkurve_amd import _capi, fitsio
from lightkurve_amd import device as D
from lightkurve_amd.device import DeviceBuffer, DeviceLightCurveBatch
from oracle import np_oracle as O

import regress_rows_cases as C

pytestmark = pytest.mark.gpu


def run(rg, **kw):
    kw.setdefault("err", rg.err)
    kw.setdefault("cadence_mask", rg.cm)
    return _capi.regress_shared_rows_batch(rg.X, rg.y, rg.n_off, rg.rows, **kw)


def resident(rg, grid, with_quality=True):
    """The ragged batch in HBM: times of the kept rows, cadence numbers grid[rows_b], quality = the row index."""
    t = np.linspace(0, 30, rg.N)
    dev = DeviceLightCurveBatch.from_arrays(t[rg.rows], rg.y, rg.err, rg.n_off, cadenceno=grid[rg.rows])
    if with_quality:
        dev.d_quality, k = D._upload(dev.handle, rg.rows, dev.stream, np.int32)
        dev._keep.append(k)
    return dev, t


# ---------------------------------------------------------------- 1. generated batches vs the oracle
@pytest.mark.parametrize("seed,B,N,K", C.CONFIGS)
def test_generated_ragged_batches_vs_oracle(seed, B, N, K):
    rg, refs = C.problem(seed, B, N, K)
    r = run(rg)
    ntot = int(rg.n_off[-1])
    assert r["model"].shape == (ntot,) and r["outlier_mask"].shape == (ntot,) and r["coefficients"].shape == (B, K)
    print("cadences per target %d..%d; clipped per target:" % (np.diff(rg.n_off).min(), np.diff(rg.n_off).max()),
          sorted(set(int(ref["outlier_mask"].sum()) for ref in refs)), "max |model - ref| / std:",
          max(np.max(np.abs(r["model"][rg.sl(b)] - refs[b]["model"])) / np.std(rg.y[rg.sl(b)]) for b in range(B)))
    C.check(r, rg, refs)


@pytest.mark.parametrize("seed,B,N,K", C.CONFIGS[:2])
def test_without_errors(seed, B, N, K):
    rg, _ = C.problem(seed, B, N, K)
    C.check(run(rg, err=None), rg, rg.refs(with_err=False))


@pytest.mark.parametrize("seed,B,N,K", [C.CONFIGS[0], C.CONFIGS[3]])
def test_priors_on_every_second_column_different_per_target(seed, B, N, K):
    rg, _ = C.problem(seed, B, N, K)
    rng = np.random.default_rng(111)
    mu = np.zeros((B, K))
    mu[:, ::2] = rng.normal(0, 1e-3, (B, (K + 1) // 2))
    sg = np.full((B, K), np.inf)
    sg[:, ::2] = 0.05
    C.check(run(rg, prior_mu=mu, prior_sigma=sg), rg, rg.refs(mu=mu, sg=sg))
    with pytest.raises(ValueError, match="both"):
        run(rg, prior_mu=mu)


def test_coefficient_covariance_vs_oracle():
    """rtol 1e-6 per element; the absolute floor is what an inverse can carry at all: an element is determined to
    cond(A) eps of the matrix's scale sqrt(C_ii C_jj) (cond <= 3.1e3: 7e-13), taken 100 times wider."""
    rg, refs = C.problem(*C.CONFIGS[0])
    r = run(rg, want_cov=True)
    C.check(r, rg, refs)
    for b, o in enumerate(refs):
        ref = o["coefficients_cov"]
        scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
        assert np.all(np.abs(r["coefficients_cov"][b] - ref) <= 1e-6 * np.abs(ref) + 1e-10 * scale), b


# ---------------------------------------------------------------- 2. full presence: the bits of the uniform path
@pytest.mark.parametrize("seed,B,N,K", [C.CONFIGS[0], C.CONFIGS[3]])
def test_full_presence_is_bit_identical_to_the_uniform_path(seed, B, N, K):
    rg, _ = C.problem(seed, B, N, K)
    X, y, err, cm = rg.X, rg.y2, rg.err2, rg.cm2
    ref = _capi.regress_shared_batch(X, y, err=err, cadence_mask=cm, want_cov=True)
    r = _capi.regress_shared_rows_batch(X, y.ravel(), np.arange(B + 1) * N, np.tile(np.arange(N, dtype=np.int32), B), err=err.ravel(),
                                        cadence_mask=cm.ravel(), want_cov=True)
    assert np.array_equal(r["coefficients"], ref["coefficients"])
    assert np.array_equal(r["model"].reshape(B, N), ref["model"])
    assert np.array_equal(r["outlier_mask"].reshape(B, N), ref["outlier_mask"])
    assert np.array_equal(r["coefficients_cov"], ref["coefficients_cov"])


def test_ragged_ridge_prior_on_a_uniform_batch_is_bit_identical():
    rg, _ = C.problem(*C.CONFIGS[0])
    B, N, K = rg.B, rg.N, rg.K
    dev = DeviceLightCurveBatch.from_arrays(np.tile(np.linspace(0, 30, N), B), rg.y2.ravel(), rg.err2.ravel(), np.arange(B + 1) * N)
    alphas = np.random.default_rng(5).uniform(1e-5, 2.0, B) * np.where(np.arange(B) % 3 == 0, -1.0, 1.0)
    for alpha, arr in ((1e-4, None), (None, alphas)):
        keep = []
        a = [d.download(np.float64, B * K, stream=dev.stream) for d in dev._ridge_prior(N, K, alpha, arr, keep)]
        b = [d.download(np.float64, B * K, stream=dev.stream) for d in dev._ridge_prior(None, K, alpha, arr, keep)]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        want = np.median(rg.err2, axis=1) / np.sqrt(np.abs(alphas if arr is not None else alpha))
        assert np.array_equal(b[1].reshape(B, K), np.repeat(want[:, None], K, axis=1)) and not b[0].any()
    # the host-pointer flavour on the ragged batch: numpy's median over each target's own cadences
    mu, sg = _capi.ridge_prior_rows_batch(rg.err, rg.n_off, K, alphas)
    want = np.array([np.median(rg.err[rg.sl(b)]) for b in range(B)]) / np.sqrt(np.abs(alphas))
    assert np.array_equal(sg, np.repeat(want[:, None], K, axis=1)) and not mu.any()


# ---------------------------------------------------------------- 3. neighbours and grid padding
def test_a_target_alone_in_the_batch_and_on_a_padded_grid():
    rg, refs = C.problem(*C.CONFIGS[0])
    full = run(rg, want_cov=True)
    rng = np.random.default_rng(77)
    for b in (1, 2, 5, 36):          # leading slices absent, trailing slices absent, every row, the last (partial) tile
        s = rg.sl(b)
        one = _capi.regress_shared_rows_batch(rg.X, rg.y[s], [0, s.stop - s.start], rg.rows[s], err=rg.err[s],
                                              cadence_mask=rg.cm[s], want_cov=True)
        assert np.array_equal(one["coefficients"][0], full["coefficients"][b]), b
        assert np.array_equal(one["model"], full["model"][s]) and np.array_equal(one["outlier_mask"], full["outlier_mask"][s]), b
        assert np.array_equal(one["coefficients_cov"][0], full["coefficients_cov"][b]), b
    # 21 rows that no target has, appended: 1024 rows split like 1003 (four slices of 256) -> the same bytes
    X21 = np.vstack([rg.X, rng.normal(0, 1, (21, rg.K))])
    pad = _capi.regress_shared_rows_batch(X21, rg.y, rg.n_off, rg.rows, err=rg.err, cadence_mask=rg.cm, want_cov=True)
    for k in full:
        assert np.array_equal(pad[k], full[k]), k
    # 100 appended rows move the slice bounds (five slices of 224): masks identical, the rest to the house tolerances
    X100 = np.vstack([rg.X, rng.normal(0, 1, (100, rg.K))])
    pad = _capi.regress_shared_rows_batch(X100, rg.y, rg.n_off, rg.rows, err=rg.err, cadence_mask=rg.cm)
    assert np.array_equal(pad["outlier_mask"], full["outlier_mask"])
    C.check(pad, rg, refs)


# ---------------------------------------------------------------- 4. align
def test_align_rows_and_pos_vs_searchsorted():
    rng = np.random.default_rng(8)
    Nx, B = 700, 19
    grid = (5000 + 3 * np.sort(rng.choice(1000, Nx, replace=False))).astype(np.int32)     # an offset and gaps (never c + 1)
    sel = [np.sort(rng.choice(Nx, int(n), replace=False)) for n in rng.integers(1, Nx + 1, B)]
    sel[3] = np.arange(Nx)
    sel[4] = np.array([Nx - 1])
    sel[7] = np.arange(0, Nx, 2)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sel])])
    cad = np.concatenate([grid[s] for s in sel])
    rows, pos = _capi.align_rows_batch(cad, off, grid, want_pos=True)
    assert np.array_equal(rows, np.searchsorted(grid, cad)) and np.array_equal(rows, np.concatenate(sel))
    want = np.full((B, Nx), -1, dtype=np.int32)
    for b, s in enumerate(sel):
        want[b, s] = np.arange(len(s))
    assert np.array_equal(pos, want)
    assert np.array_equal(_capi.align_rows_batch(cad, off, grid), rows)
    # a cadence that is not on the grid: the call fails and names the first such target
    bad = cad.copy()
    bad[off[7] + 2] += 1                                                           # between two grid values: still increasing
    bad[off[12]] = 4999                                                            # before the grid's first
    with pytest.raises(ValueError, match=r"target 7 .*not on the grid"):
        _capi.align_rows_batch(bad, off, grid)
    beyond = cad.copy()
    beyond[off[5] - 1] = 9000                                                      # target 4's only cadence, past the grid's last
    with pytest.raises(ValueError, match=r"target 4 .*not on the grid"):
        _capi.align_rows_batch(beyond, off, grid)
    swapped = cad.copy()
    swapped[off[3] + 10], swapped[off[3] + 11] = cad[off[3] + 11], cad[off[3] + 10]
    with pytest.raises(ValueError, match=r"target 3.*strictly increasing"):
        _capi.align_rows_batch(swapped, off, grid)
    with pytest.raises(ValueError, match="grid.*strictly increasing"):
        _capi.align_rows_batch(cad, off, grid[::-1].copy())


def test_rows_that_do_not_increase_or_leave_the_grid_raise():
    rg, _ = C.problem(*C.CONFIGS[1])
    for edit in ("equal", "past"):
        rows = rg.rows.copy()
        i = int(rg.n_off[6]) + 40
        rows[i] = rows[i - 1] if edit == "equal" else rg.N
        with pytest.raises(ValueError, match=r"target 6.*strictly increasing"):
            _capi.regress_shared_rows_batch(rg.X, rg.y, rg.n_off, rows, err=rg.err)


def test_cadences_off_the_grid_are_dropped_with_the_count_in_meta():
    rg, _ = C.problem(*C.CONFIGS[1])
    B, N = rg.B, rg.N
    grid_all = 1000 + 2 * np.arange(N, dtype=np.int32)
    dev, t = resident(rg, grid_all)
    # the grid loses 9 rows: the targets that have them lose those cadences, as CotrendingBasisVectors.align drops them
    gone = np.array([0, 1, 200, 201, 202, 300, 400, 515, 516])
    on = np.setdiff1d(np.arange(N), gone)
    grid, X = grid_all[on], rg.X[on]
    cm_dev, _k = D._upload(dev.handle, rg.cm.astype(np.uint8), dev.stream, np.uint8)
    for cm in (rg.cm, cm_dev):
        out, d_outl, d_w = dev.regression_correct(X, cadence_mask=cm, cadenceno=grid)
        keep = ~np.isin(rg.rows, gone)
        want_drop = [int((~keep[rg.sl(b)]).sum()) for b in range(B)]
        assert [m["CADENCES_NOT_ON_GRID"] for m in out.meta] == want_drop and max(want_drop) > 0
        assert "CADENCES_NOT_ON_GRID" not in dev.meta[0]
        assert np.array_equal(np.diff(out.n_off), np.diff(rg.n_off) - want_drop)
        assert np.array_equal(out.cadenceno_host(), grid_all[rg.rows][keep]) and np.array_equal(out.time_host(), t[rg.rows][keep])
        w = d_w.download(np.float64, B * rg.K, stream=dev.stream).reshape(B, rg.K)
        outl = d_outl.download(np.uint8, int(out.n_off[-1]), stream=dev.stream).astype(bool)
        corrected = out.flux_host()
        for b in range(B):
            s, k = rg.sl(b), keep[rg.sl(b)]
            rb = np.searchsorted(on, rg.rows[s][k])
            yb, eb, cb = rg.y[s][k], rg.err[s][k], rg.cm[s][k]
            assert C.clip_margin(X[rb], yb, eb, cb) > C.MIN_MARGIN_SD
            ref = O.regression_correct(X[rb], yb, eb, cb)
            so = slice(int(out.n_off[b]), int(out.n_off[b + 1]))
            assert np.array_equal(outl[so], ref["outlier_mask"]), b
            assert np.max(np.abs(corrected[so] - ref["corrected"])) / np.std(yb) < 1e-9, b
            assert np.allclose(w[b], ref["coefficients"], rtol=1e-6, atol=1e-9), b


# ---------------------------------------------------------------- 5. cbv_correct on a ragged resident batch
def test_cbv_correct_on_a_ragged_resident_batch():
    rg, _ = C.problem(*C.CONFIGS[0])
    B, N, K = rg.B, rg.N, rg.K
    grid = 31000 + np.arange(N, dtype=np.int32) * 3
    dev, t = resident(rg, grid)
    cbvs = rg.X[:, :16]
    alphas = np.random.default_rng(6).uniform(1e-5, 1e-3, B)
    for alpha in (1e-4, alphas):
        a = np.broadcast_to(alpha, (B,))
        sg = np.array([np.full(K, np.median(rg.err[rg.sl(b)]) / np.sqrt(a[b])) for b in range(B)])
        refs = rg.refs(mu=np.zeros((B, K)), sg=sg)
        corrected, outl, coef = dev.cbv_correct(cbvs, cbv_indices="ALL", alpha=alpha, cadence_mask=rg.cm, cadenceno=grid, to_host=True)
        assert len(corrected) == B and len(outl) == B and coef.shape == (B, K)
        # (y - (y - model) differs from the model by roundings of y's size, 1e-13 std(y): far inside the 1e-9 of check())
        C.check(dict(coefficients=coef, model=rg.y - np.concatenate(corrected), outlier_mask=np.concatenate(outl)), rg, refs)
        for b in range(B):
            assert np.max(np.abs(corrected[b] - refs[b]["corrected"])) / np.std(rg.y[rg.sl(b)]) < 1e-9, b
        out, d_outl, d_w = dev.cbv_correct(cbvs, cbv_indices="ALL", alpha=alpha, cadence_mask=rg.cm, cadenceno=grid)
        assert isinstance(d_outl, DeviceBuffer) and isinstance(d_w, DeviceBuffer)
        assert np.array_equal(out.n_off, rg.n_off) and np.array_equal(out.flux_host(), np.concatenate(corrected))
        assert np.array_equal(out.time_host(), t[rg.rows]) and np.array_equal(out.flux_err_host(), rg.err)
        assert np.array_equal(out.quality_host(), rg.rows) and np.array_equal(out.cadenceno_host(), grid[rg.rows])
        assert np.array_equal(d_w.download(np.float64, B * K, stream=dev.stream).reshape(B, K), coef)
        assert np.array_equal(d_outl.download(np.uint8, int(rg.n_off[-1]), stream=dev.stream).astype(bool), np.concatenate(outl))
        assert all(m["CADENCES_NOT_ON_GRID"] == 0 for m in out.meta)
    # rows= gives what cadenceno= gives, bit for bit; the host convenience too
    mu = np.zeros((B, K))
    a = dev.regression_correct(rg.X, prior_mu=mu, prior_sigma=sg, cadence_mask=rg.cm, rows=rg.rows, to_host=True)
    assert np.array_equal(np.concatenate(a[0]), np.concatenate(corrected)) and np.array_equal(a[2], coef)

    class HostLC(object):
        pass
    lcs = []
    for b in range(B):
        lc = HostLC()
        s = rg.sl(b)
        lc.time, lc.flux, lc.flux_err, lc.cadenceno = t[rg.rows[s]], rg.y[s], rg.err[s], grid[rg.rows[s]]
        lcs.append(lc)
    from lightkurve_amd.batch import cbv_correct_batch
    flux, coef2, outl2, kept = cbv_correct_batch(lcs, cbvs, grid, cbv_indices="ALL", alpha=alphas,
                                                 cadence_masks=[rg.cm[rg.sl(b)] for b in range(B)])
    assert np.array_equal(coef2, coef) and all(k.all() for k in kept)
    assert np.array_equal(np.concatenate(flux), np.concatenate(corrected))


# ---------------------------------------------------------------- 6. composition with the cleaning chain
def test_remove_outliers_then_cbv_correct_equals_the_staged_route():
    rg, _ = C.problem(*C.CONFIGS[2])
    B, N, K = rg.B, rg.N, rg.K
    grid = 7 + np.arange(N, dtype=np.int32)
    dev, t = resident(rg, grid)
    clean, d_mask = dev.remove_outliers(sigma_upper=3, return_mask=True)
    removed = d_mask.download(np.uint8, int(rg.n_off[-1]), stream=dev.stream).astype(bool)
    assert removed.any() and clean.n_cadences == int((~removed).sum())
    cbvs = rg.X[:, :K - 1]
    out, d_outl, d_w = clean.cbv_correct(cbvs, cbv_indices="ALL", alpha=1e-4, cadenceno=grid)
    host = out.to_host()
    assert np.array_equal(host.cadenceno, grid[rg.rows][~removed]) and np.array_equal(host.quality, rg.rows[~removed])
    w = d_w.download(np.float64, B * K, stream=dev.stream).reshape(B, K)
    outl = d_outl.download(np.uint8, clean.n_cadences, stream=dev.stream).astype(bool)
    for b in range(B):
        s, k = rg.sl(b), ~removed[rg.sl(b)]
        yb, eb, rb = rg.y[s][k], rg.err[s][k], rg.rows[s][k]
        sg = np.full(K, np.median(eb) / np.sqrt(1e-4))
        assert C.clip_margin(rg.X[rb], yb, eb, None, np.zeros(K), sg) > C.MIN_MARGIN_SD
        ref = O.regression_correct(rg.X[rb], yb, eb, None, np.zeros(K), sg)
        so = slice(int(host.n_off[b]), int(host.n_off[b + 1]))
        assert np.array_equal(outl[so], ref["outlier_mask"]), b
        assert np.max(np.abs(host.flux[so] - ref["corrected"])) / np.std(yb) < 1e-9, b
        assert np.allclose(w[b], ref["coefficients"], rtol=1e-6, atol=1e-9), b


# ---------------------------------------------------------------- 7. from_fits
def test_from_fits_fills_the_cadence_numbers_of_the_kept_rows(golden):
    g = golden("fits_ingest")
    fdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fits")
    names, tags = ("kepler_llc.fits", "tess_lc.fits"), ("kepler_default", "tess_default")
    paths = [os.path.join(fdir, n) for n in names]
    dev = DeviceLightCurveBatch.from_fits(paths)
    cad = dev.cadenceno_host()
    assert cad.dtype == np.int32 and cad.shape == (dev.n_cadences,)
    for b, (path, tag) in enumerate(zip(paths, tags)):
        tab = fitsio.read_fits_table(path)
        off = tab.columns["time"][0]
        rec = np.asarray(tab.raw, dtype=np.uint8).reshape(tab.n_rows, tab.row_bytes)
        time = np.ascontiguousarray(rec[:, off:off + 8]).view(">f8").ravel()
        src = np.flatnonzero(np.isin(time, g[tag + "_time"]))
        assert np.array_equal(time[src], g[tag + "_time"])
        s = slice(int(dev.n_off[b]), int(dev.n_off[b + 1]))
        assert len(src) < tab.n_rows and np.array_equal(cad[s], 1000 + src), tag
    # carried through the cleaning chain, in step with the cadences that survive
    flux = dev.flux_host()
    clean = dev.remove_nans()
    assert np.array_equal(clean.cadenceno_host(), cad[~np.isnan(flux)]) and clean.n_cadences < dev.n_cadences
    assert np.array_equal(clean.normalize().flatten(11).cadenceno_host(), clean.cadenceno_host())
    pick = np.arange(clean.n_cadences) % 3 != 0
    assert np.array_equal(clean.select(pick).cadenceno_host(), clean.cadenceno_host()[pick])
    assert np.array_equal(clean.select(pick).quality_host(), clean.quality_host()[pick])
    assert np.array_equal(DeviceLightCurveBatch.from_batch(clean.to_host()).cadenceno_host(), clean.cadenceno_host())
    # a file without the column: the batch carries none
    assert DeviceLightCurveBatch.from_arrays(np.arange(5.0), np.ones(5), np.ones(5), [0, 5]).cadenceno_host() is None


# ---------------------------------------------------------------- 8. degenerate targets
def test_one_target_five_cadences_one_column():
    rng = np.random.default_rng(1)
    X = np.ones((9, 1))
    rows = np.array([0, 2, 3, 7, 8], dtype=np.int32)
    y = 3.0 + rng.normal(0, 1e-3, 5)
    err = np.full(5, 1e-3)
    r = _capi.regress_shared_rows_batch(X, y, [0, 5], rows, err=err)
    ref = O.regression_correct(X[rows], y, err)
    assert np.array_equal(r["outlier_mask"], ref["outlier_mask"])
    assert np.max(np.abs(r["model"] - ref["model"])) / np.std(y) < 1e-9
    assert np.allclose(r["coefficients"][0], ref["coefficients"], rtol=1e-6, atol=1e-9)


def test_target_with_an_empty_ragged_cadence_mask_returns_its_prior():
    rg, _ = C.problem(*C.CONFIGS[1])       # B = 19: not a multiple of 16
    B, K = rg.B, rg.K
    cm = rg.cm.copy()
    cm[rg.sl(4)] = False
    mu = np.tile(np.array([0.5, -0.25, 1.0]), (B, 1))
    sg = np.full((B, K), 10.0)
    r = run(rg, cadence_mask=cm, prior_mu=mu, prior_sigma=sg)
    assert np.allclose(r["coefficients"][4], mu[4], rtol=1e-12, atol=0)
    others = [b for b in range(B) if b != 4]
    refs = []
    for b in others:
        s = rg.sl(b)
        assert C.clip_margin(rg.X[rg.rows_b[b]], rg.y[s], rg.err[s], rg.cm[s], mu[b], sg[b]) > C.MIN_MARGIN_SD
        refs.append(O.regression_correct(rg.X[rg.rows_b[b]], rg.y[s], rg.err[s], rg.cm[s], mu[b], sg[b]))
    C.check(r, rg, refs, targets=others)


def test_one_column_past_the_bound_is_refused_and_names_the_other_entry_point():
    rng = np.random.default_rng(2)
    X = rng.normal(0, 1, (200, 65))
    y = rng.normal(1, 1e-3, 3 * 150)
    rows = np.tile(np.arange(150, dtype=np.int32), 3)
    with pytest.raises(ValueError, match="lk_regress_batch") as ei:
        _capi.regress_shared_rows_batch(X, y, [0, 150, 300, 450], rows)
    assert "64" in str(ei.value)


def test_non_finite_flux_or_a_zero_error_is_an_error():
    rg, _ = C.problem(*C.CONFIGS[1])
    bad = rg.y.copy()
    bad[int(rg.n_off[7]) + 100] = np.nan
    with pytest.raises(ValueError, match="NaNs in the flux"):
        _capi.regress_shared_rows_batch(rg.X, bad, rg.n_off, rg.rows, err=rg.err, cadence_mask=rg.cm)
    bad = rg.err.copy()
    bad[-1] = 0.0
    with pytest.raises(ValueError, match="flux errors"):
        run(rg, err=bad)
