"""GPU: the per-target ridge search of a resident batch (DeviceLightCurveBatch.cbv_correct_optimized) and the three device-side
splits under it: one ridge penalty per target (lk_ridge_prior_alphas_batch_dev), the under-fitting metric against prepared
neighbour rows (lk_underfit_rows_*, lk_underfit_against_rows_batch_dev) and the over-fitting metric as a session
(lk_overfit_session_*).

Fields: overfit_cases.field(N, B=6) with its three systematics as the basis vectors (cbv_indices = [1, 2, 3]); the explicit
neighbour batch is the good correction (variant b) of a four-target field.

Tolerances.  Wherever two calls run the same kernels on the same numbers the assertion is bit equality.  Two are not: the
rows entry against the repository's ``underfit_metric_neighbors`` (a correct kernel is within about n 2^-53 ~ 3e-14), and the
session against the unsplit over-fitting metric (|mean_unc| * nanmean(LS(normal)) against nanmean(LS(normal * mean_unc)): a few
ulp of a number of order one); both are asserted < 1e-9 absolute (the house rule) and their maxima printed."""
import ctypes
import functools

import numpy as np
import pytest

import overfit_cases as C
import underfit_cases as U
from lightkurve_amd import _capi
from lightkurve_amd.correctors.cbvcorrector import _leaky, minimize_scalar_bounded
from lightkurve_amd.device import DeviceBuffer, DeviceLightCurveBatch

pytestmark = pytest.mark.gpu
TOL = 1e-9
B, BN = 6, 4
IDX = [1, 2, 3]
RNG = dict(seed=7, first_target=0, stream_id=3)
_vp = ctypes.c_void_p


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def resident(t, y, err):
    """A NaN-free resident batch of the rows of y on the shared times t."""
    nb, N = y.shape
    dev = DeviceLightCurveBatch.from_arrays(np.tile(t, nb), np.ascontiguousarray(y).reshape(-1), np.ascontiguousarray(err).reshape(-1),
                                            np.arange(nb + 1) * N)
    return dev.remove_nans()


def neighbour_rows(N):
    """The flux of the explicit neighbour batch: BN well-corrected targets of another field on the same cadences."""
    return C.field(N, B=BN, seed=12)["variants"]["b"]


def neighbour_batch(N):
    f = C.field(N, B=BN, seed=12)
    return resident(f["t"], neighbour_rows(N), f["err"])


# rows of the neighbour batch: one padded slot, and rows 1 and 3 list their own number (a row of the OTHER batch)
NEIGHBORS = np.array([[0, 1, 2], [1, 3, -1], [3, 2, 0], [2, 3, 1], [-1, 0, 3], [1, 0, 2]], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ 1. one alpha per target
def test_per_target_alpha_gives_the_rows_of_the_scalar_calls():
    N = 65
    f = C.field(N, B=B)
    dev = resident(f["t"], f["y"], f["err"])
    cbvs = C.systematics(N)
    alphas = np.array([1e-4, 1e-2, 1, 1e2, 1e4, 3.7])
    cor, outl, w = dev.cbv_correct(cbvs, cbv_indices=IDX, alpha=alphas, to_host=True)
    for b, a in enumerate(alphas):
        c1, o1, w1 = dev.cbv_correct(cbvs, cbv_indices=IDX, alpha=float(a), to_host=True)
        assert same_bits(cor[b], c1[b]) and np.array_equal(outl[b], o1[b]) and same_bits(w[b], w1[b]), b
    assert not same_bits(w[0], dev.cbv_correct(cbvs, cbv_indices=IDX, alpha=1e4, to_host=True)[2][0])   # alpha does matter
    # a list and a negative penalty (|alpha|) go the same way
    c2 = dev.cbv_correct(cbvs, cbv_indices=IDX, alpha=list(-alphas), to_host=True)[0]
    assert same_bits(c2, cor)


# ------------------------------------------------------------------------------------------------ 2. the rows entry
def mirror_against(y, ynb, nb, cm, t):
    """``underfit_metric_neighbors`` per target with the neighbours taken from the rows of ynb (underfit_cases.mirror on the
    stacked array, the neighbour rows listing nothing themselves)."""
    nt = len(y)
    table = np.full((nt + len(ynb), nb.shape[1]), -1, dtype=np.int64)
    table[:nt] = np.where(nb >= 0, nb + nt, -1)
    m, c = U.mirror(np.vstack([y, ynb]), table, cm, t)
    return m[:nt], c[:nt]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N", [127, 128, 129])
def test_rows_entry_on_the_pitch_edge(N, masked):
    f = C.field(N, B=B)
    t, y, err = f["t"], f["y"], f["err"]
    cm = C.masks(N)[0] if masked else None
    assert cm is None or cm.sum() % 2 == 1
    dev = resident(t, y, err)
    # the batch as its own neighbour batch: the bits of today's call
    own = np.array([[1, 2, 3], [0, 5, -1], [4, 3, 1], [5, 0, 2], [-1, 2, 0], [3, 4, 1]], dtype=np.int32)
    m0, c0 = dev.under_fitting_metric(own, cadence_mask=cm, return_correlations=True)
    m1, c1 = dev.under_fitting_metric(own, cadence_mask=cm, return_correlations=True, neighbor_batch=dev)
    assert same_bits(m0, m1) and same_bits(c0, c1)
    assert same_bits(dev.under_fitting_metric(own, cadence_mask=cm, neighbor_batch=dev), m0)
    assert all(k is not dev for k in dev._keep)      # a batch must not hold itself: its buffers would wait for the collector
    # another batch of BN != B rows
    ynb = neighbour_rows(N)
    m2, c2 = dev.under_fitting_metric(NEIGHBORS, cadence_mask=cm, return_correlations=True, neighbor_batch=neighbour_batch(N))
    ref_m, ref_c = mirror_against(y, ynb, NEIGHBORS, cm, t)
    pad = NEIGHBORS < 0
    assert c2.shape == NEIGHBORS.shape and np.array_equal(np.isnan(c2), pad)
    err_m, err_c = float(np.max(np.abs(m2 - ref_m))), float(np.max(np.abs(c2[~pad] - ref_c[~pad])))
    print("N = %d masked = %s: max |metric - mirror| %.3e   max |corr - mirror| %.3e" % (N, masked, err_m, err_c))
    assert err_m < TOL and err_c < TOL
    assert not same_bits(m2, m0)


# ------------------------------------------------------------------------------------------------ 3. the session
class Session(object):
    """lk_overfit_session_* by raw calls on DeviceBuffers."""

    def __init__(self, orig, n_samples, cm, seed, first_target, stream_id):
        self.h, self.B = orig.handle, len(orig)
        self.N = orig.n_cadences // self.B
        t = orig.time_host()[:self.N]
        self.keep_idx, self.n, _ = _capi.overfit_arguments(self.N, n_samples, cm, None, seed, first_target, stream_id, self.B)
        self.grid = _capi.overfit_grid(_capi.overfit_default_grid(t if cm is None else t[cm]))
        self.ns = n_samples
        self.d_keep = None
        if self.keep_idx is not None:
            self.d_keep = DeviceBuffer(self.h, self.keep_idx.nbytes)
            self.d_keep.upload(self.keep_idx)
        nbytes, rounds = ctypes.c_int64(0), ctypes.c_int(0)
        _capi._check(_capi._lib.lk_overfit_session_bytes(self.B, self.n, self.grid[2], n_samples, 0, ctypes.byref(nbytes),
                                                         ctypes.byref(rounds)))
        assert nbytes.value > 0 and 1 <= rounds.value <= n_samples
        self.nbytes = nbytes.value
        self.block = DeviceBuffer(self.h, self.nbytes)
        self.d_metric = DeviceBuffer(self.h, self.B * 8)
        self.orig = orig
        _capi._check(_capi._lib.lk_overfit_session_begin_dev(
            self.h._h, self.B, self.N, _vp(orig.d_time.ptr), _vp(orig.d_flux.ptr), self.n, self._keep(), self.grid[0], self.grid[1],
            self.grid[2], n_samples, seed, first_target, stream_id, _vp(self.block.ptr), self.nbytes, None))

    def _keep(self):
        return _vp(self.d_keep.ptr if self.d_keep is not None else None)

    def eval(self, cor):
        _capi._check(_capi._lib.lk_overfit_session_eval_dev(
            self.h._h, self.B, self.N, _vp(cor.d_flux.ptr), _vp(cor.d_flux_err.ptr), self.n, self._keep(), self.grid[0],
            self.grid[1], self.grid[2], self.ns, _vp(self.block.ptr), self.nbytes, _vp(self.d_metric.ptr), None))
        return self.d_metric.download(np.float64, self.B)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("N", [5, 64, 65, 129])
def test_session_against_the_unsplit_metric(N, masked):
    f = C.field(N, B=B)
    t, y, err = f["t"], f["y"], f["err"]
    cm = C.masks(N)[0] if masked else None
    orig = resident(t, y, err)
    cors = {name: resident(t, f["variants"][name], err) for name in ("a", "b", "c1", "c4")}
    worst = 0.0
    for ns in (1, 3):
        sess = Session(orig, ns, cm, 7, 2, 3)
        first = {}
        for name in ("b", "c4", "c1", "a"):
            got = sess.eval(cors[name])
            ref = cors[name].over_fitting_metric(orig, n_samples=ns, cadence_mask=cm, seed=7, first_target=2, stream_id=3)
            assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref)), (name, ns, got, ref)
            worst = max(worst, float(np.max(np.abs(got - ref))))
            first[name] = got
        assert np.all(first["a"] == 1.0)
        # an evaluation leaves nothing behind: b again, after c4, c1 and a on the same session
        assert same_bits(sess.eval(cors["b"]), first["b"])
        assert not same_bits(first["b"], first["c4"])
    print("N = %d masked = %s: max |session - unsplit| = %.3e" % (N, masked, worst))
    assert worst < TOL


# ------------------------------------------------------------------------------------------------ 4. the search, by its trace
N_SEARCH = 129


def search_inputs():
    f = C.field(N_SEARCH, B=B)
    return f, C.systematics(N_SEARCH)


def run_search(rows=slice(None), first_target=0, **kw):
    f, cbvs = search_inputs()
    dev = resident(f["t"], f["y"][rows], f["err"][rows])
    args = dict(neighbors=NEIGHBORS[rows], neighbor_batch=neighbour_batch(N_SEARCH), cbv_indices=IDX, seed=RNG["seed"],
                first_target=first_target, stream_id=RNG["stream_id"], return_trace=True)
    args.update(kw)
    out, info = dev.cbv_correct_optimized(cbvs, **args)
    return dev, out, info, out.flux_host().reshape(len(dev), N_SEARCH).copy()


@functools.lru_cache(maxsize=None)
def full_run():
    """The search of the whole field, shared by the tests that read it (treated as read-only)."""
    return run_search()


def test_search_follows_the_scalar_search_on_its_own_trace():
    dev, out, info, flux = full_run()
    f, cbvs = search_inputs()
    nbatch = neighbour_batch(N_SEARCH)
    tr = info["trace"]
    steps = tr["alpha"].shape[0]
    assert tr["alpha"].shape == tr["over"].shape == tr["under"].shape == (steps, B)
    assert np.all(info["status"] == 0) and steps == info["nfev"].max() and info["nfev"].min() >= 3
    print("evaluations per target:", info["nfev"], " alpha:", info["alpha"])
    # (a) every step again through the public calls
    worst = 0.0
    for i in range(steps):
        cor = dev.cbv_correct(cbvs, cbv_indices=IDX, alpha=tr["alpha"][i])[0]
        over = cor.over_fitting_metric(dev, n_samples=1, **RNG)
        under = cor.under_fitting_metric(NEIGHBORS, neighbor_batch=nbatch)
        assert np.all(np.isfinite(over)) and np.all(np.isfinite(tr["over"][i])), i
        worst = max(worst, float(np.max(np.abs(over - tr["over"][i]))))
        assert same_bits(under, tr["under"][i]), i
    print("max |session over - unsplit over| along the trace = %.3e over %d steps" % (worst, steps))
    assert worst < TOL
    # (b) the scalar search, fed the traced objective, asks for the traced abscissae; (c) the optimum is the best value seen
    for b in range(B):
        obj = [-(_leaky(tr["over"][i, b], 0.5) + _leaky(tr["under"][i, b], 0.5)) for i in range(steps)]
        asked = []

        def replay(a):
            asked.append(float(a))
            return obj[len(asked) - 1]

        r = minimize_scalar_bounded(replay, (1e-4, 1e4), maxiter=100)
        nf = int(info["nfev"][b])
        assert r["nfev"] == nf == len(asked) and r["status"] == info["status"][b]
        assert same_bits(asked, tr["alpha"][:nf, b]) and same_bits(r["x"], info["alpha"][b])
        assert np.all(bits(tr["alpha"][nf:, b]) == bits(info["alpha"][b]))          # a finished target waits at its optimum
        assert same_bits(r["fun"], info["objective"][b]) and np.all(info["objective"][b] <= np.array(obj[:nf]))
    # (d) what comes back is the fit at the optimum and its scores
    cor = dev.cbv_correct(cbvs, cbv_indices=IDX, alpha=info["alpha"])[0]
    assert same_bits(cor.flux_host().reshape(B, N_SEARCH), flux)
    assert same_bits(cor.over_fitting_metric(dev, n_samples=10, **RNG), info["over_fitting_score"])
    assert same_bits(cor.under_fitting_metric(NEIGHBORS, neighbor_batch=nbatch), info["under_fitting_score"])
    assert np.all((info["over_fitting_score"] > 0) & (info["over_fitting_score"] <= 1))
    assert np.all((info["under_fitting_score"] > 0) & (info["under_fitting_score"] <= 1))


def same_run(a, b, rows=slice(None)):
    (_, _, ia, fa), (_, _, ib, fb) = a, b
    for k in ("alpha", "over_fitting_score", "under_fitting_score", "objective"):
        assert same_bits(ia[k][rows], ib[k]), k
    assert np.array_equal(ia["nfev"][rows], ib["nfev"]) and np.array_equal(ia["status"][rows], ib["status"])
    assert same_bits(fa[rows], fb)


def test_search_gives_the_same_bits_twice():
    again = run_search()
    same_run(full_run(), again)
    for k in ("alpha", "over", "under"):
        assert same_bits(full_run()[2]["trace"][k], again[2]["trace"][k]), k


# ------------------------------------------------------------------------------------------------ 5. independence of the batch
def test_a_target_does_not_depend_on_the_rest_of_the_batch():
    part = run_search(rows=slice(2, 5), first_target=2)
    assert np.all(part[2]["status"] == 0)
    same_run(full_run(), part, rows=slice(2, 5))


# ------------------------------------------------------------------------------------------------ 6. skipped metrics
def test_skipped_metrics_report_minus_one():
    _, _, info, _ = run_search(target_under_score=0, neighbors=None, neighbor_batch=None)
    assert np.all(info["under_fitting_score"] == -1.0) and np.all(info["trace"]["under"] == 1.0)
    assert np.all((info["over_fitting_score"] > 0) & (info["over_fitting_score"] <= 1)) and np.all(info["status"] == 0)
    _, _, info, _ = run_search(target_over_score=0)
    assert np.all(info["over_fitting_score"] == -1.0) and np.all(info["trace"]["over"] == 1.0)
    assert np.all((info["under_fitting_score"] > 0) & (info["under_fitting_score"] <= 1)) and np.all(info["status"] == 0)
    # both skipped: a constant objective, every target walks the same abscissae
    _, _, info, _ = run_search(target_over_score=0, target_under_score=-1, neighbors=None, neighbor_batch=None)
    r = minimize_scalar_bounded(lambda a: -2.0, (1e-4, 1e4), maxiter=100)
    assert np.all(info["objective"] == -2.0) and np.all(info["nfev"] == r["nfev"]) and np.all(info["status"] == r["status"])
    assert np.all(bits(info["alpha"]) == bits(r["x"]))
    assert np.all(bits(info["trace"]["alpha"]) == bits(info["trace"]["alpha"][:, :1]))
    assert np.all(info["over_fitting_score"] == -1.0) and np.all(info["under_fitting_score"] == -1.0)
