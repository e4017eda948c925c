"""No GPU: ``cotrend._ridge_search`` — the one driver of ``cbv_correct_optimized`` — on a host-only layout whose two scores are
closed-form functions of alpha, different for each of B = 3 targets.  Per target the driver must give, bit for bit, what
``minimize_scalar_bounded`` gives on that target's scalar objective; the trace, the skipped scores, ``max_iter`` and the argument
checks are the driver's own."""
import numpy as np
import pytest

from lightkurve_amd import cotrend
from lightkurve_amd.correctors.cbvcorrector import _leaky, minimize_scalar_bounded

BOUNDS = (1e-4, 1e4)


def _sigmoid(u):
    return 1.0 / (1.0 + np.exp(-u))


# (over-fitting score, under-fitting score) of each target as functions of its alpha
SCORES = [
    (lambda a: _sigmoid(-(np.log10(a) - 1.0) * 2.0), lambda a: _sigmoid((np.log10(a) + 1.0) * 1.5)),
    (lambda a: 1.0 / (1.0 + 0.5 / a), lambda a: 1.0 / (1.0 + a / 3.0)),
    (lambda a: 0.9 * np.exp(-(np.log10(a) - 2.0) ** 2 / 3.0), lambda a: 0.2 + 0.6 / (1.0 + (a / 40.0) ** 2)),
]
B = len(SCORES)


class FakeBatch(object):
    """What a layout's ``fit`` hands the driver: the alphas it was fitted at; ``synchronize`` and ``_keep`` as a batch has them."""

    def __init__(self, alphas):
        self.alphas, self._keep, self.synchronized = np.array(alphas, dtype=np.float64), [], False

    def synchronize(self):
        self.synchronized = True


class FakeLayout(object):
    """A layout that lives on the host: the operations ``_ridge_search`` asks of ``_UniformLayout`` / ``_RowsLayout``."""
    flux_errors = True
    B = B

    def __init__(self):
        self.calls = []

    def prepare(self, neighbors, neighbor_batch, stream_id, fixed):
        self.calls.append(("prepare", neighbors is not None, fixed))

    def session_begin(self, stream_id, max_scratch_bytes):
        self.calls.append(("session_begin",))

    def neighbour_rows(self, neighbor_batch, neighbor_alpha):
        self.calls.append(("neighbour_rows", neighbor_alpha))

    def fit(self, alphas=None, alpha=None):
        return FakeBatch(alphas)

    def eval_scores(self, cor, do_over, do_under, scores):
        self.calls.append(("eval", do_over, do_under))
        for b, (over, under) in enumerate(SCORES):
            if do_over:
                scores[0, b] = over(cor.alphas[b])
            if do_under:
                scores[1, b] = under(cor.alphas[b])

    def over_metric(self, cor, n_samples, stream_id, to_host, max_scratch_bytes):
        assert n_samples == 10 and to_host
        self.calls.append(("over_metric",))
        return np.array([over(a) for (over, _), a in zip(SCORES, cor.alphas)])

    def final_under(self, cor):
        self.calls.append(("final_under",))
        return np.array([under(a) for (_, under), a in zip(SCORES, cor.alphas)])

    def extra_info(self, do_under, scan=False):
        return dict(marker=do_under)

    def held(self):
        return ["held by the layout"]


class UntouchableLayout(object):
    """Any question to this layout but whether the batch has flux errors is one asked too early."""

    def __init__(self, flux_errors=True):
        self.__dict__["flux_errors"] = flux_errors

    def __getattr__(self, name):
        raise AssertionError("the layout was asked for %s before the search's own arguments were checked" % name)


def search(layout, neighbors="given", t_over=0.5, t_under=0.5, max_iter=100, alpha_bounds=BOUNDS, neighbor_alpha=1e-20, trace=True):
    return cotrend._ridge_search(layout, neighbors, None, alpha_bounds, t_over, t_under, max_iter, neighbor_alpha, 0, None, trace)


def scalar_reference(t_over, t_under, max_iter):
    """Per target: ``minimize_scalar_bounded`` on its scalar objective (a skipped score counts as 1.0) and the abscissae it visits."""
    runs = []
    for over, under in SCORES:
        xs = []

        def objective(a, over=over, under=under, xs=xs):
            xs.append(float(a))
            o = over(a) if t_over > 0 else 1.0
            u = under(a) if t_under > 0 else 1.0
            return -(_leaky(o, t_over) + _leaky(u, t_under))

        runs.append((minimize_scalar_bounded(objective, BOUNDS, maxiter=max_iter), xs))
    return runs


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("t_over,t_under", [(0.5, 0.5), (0.8, 0.3), (0.0, 0.5), (0.5, 0.0)])
@pytest.mark.parametrize("max_iter", [100, 12, 1])
def test_driver_equals_the_scalar_search_per_target(t_over, t_under, max_iter):
    ref = scalar_reference(t_over, t_under, max_iter)
    layout = FakeLayout()
    out, info = search(layout, t_over=t_over, t_under=t_under, max_iter=max_iter)
    for b, (r, xs) in enumerate(ref):
        assert bits(info["alpha"][b]) == bits(r["x"]) and bits(info["objective"][b]) == bits(r["fun"]), b
        assert info["nfev"][b] == r["nfev"] == len(xs) and info["status"][b] == r["status"], b
    steps = max(r["nfev"] for r, _ in ref)
    tr = info["trace"]
    assert tr["alpha"].shape == tr["over"].shape == tr["under"].shape == (steps, B)
    for b, (r, xs) in enumerate(ref):
        # the abscissae the scalar search visits, then the optimum again while the other targets go on
        assert np.array_equal(bits(tr["alpha"][:len(xs), b]), bits(xs)), b
        assert np.all(bits(tr["alpha"][len(xs):, b]) == bits(r["x"])), b
        over, under = SCORES[b]
        want_over = [over(a) if t_over > 0 else 1.0 for a in tr["alpha"][:, b]]
        want_under = [under(a) if t_under > 0 else 1.0 for a in tr["alpha"][:, b]]
        assert np.array_equal(bits(tr["over"][:, b]), bits(want_over)) and np.array_equal(bits(tr["under"][:, b]), bits(want_under)), b
    # the fit at the optimum and its scores; a skipped score is reported as -1.0 and nothing is asked of the layout for it
    assert np.array_equal(bits(out.alphas), bits(info["alpha"])) and out._keep == ["held by the layout"]
    names = [c[0] for c in layout.calls]
    if t_over > 0:
        assert np.array_equal(bits(info["over_fitting_score"]), bits([o(a) for (o, _), a in zip(SCORES, info["alpha"])]))
    else:
        assert np.all(info["over_fitting_score"] == -1.0) and "session_begin" not in names and "over_metric" not in names
    if t_under > 0:
        assert np.array_equal(bits(info["under_fitting_score"]), bits([u(a) for (_, u), a in zip(SCORES, info["alpha"])]))
    else:
        assert np.all(info["under_fitting_score"] == -1.0) and "neighbour_rows" not in names and "final_under" not in names
    assert layout.calls[0] == ("prepare", t_under > 0, True) and info["marker"] == (t_under > 0)
    assert names.count("eval") == steps and all(c == ("eval", t_over > 0, t_under > 0) for c in layout.calls if c[0] == "eval")
    if max_iter == 1:
        assert np.all(info["status"] == 1)
    elif max_iter == 100:
        assert np.all(info["status"] == 0) and len({r["nfev"] for r, _ in ref}) > 1       # the searches end at different steps


def test_without_a_trace_info_has_none():
    assert "trace" not in search(FakeLayout(), trace=False)[1]


def test_the_searchs_own_arguments_are_checked_before_the_layout_is_asked_for_anything():
    for bad in [(1e-4, np.inf), (np.nan, 1.0), (10.0, 1.0)]:
        with pytest.raises(ValueError, match="alpha_bounds"):
            search(UntouchableLayout(), alpha_bounds=bad)
    with pytest.raises(ValueError, match="max_iter must be >= 1"):
        search(UntouchableLayout(), max_iter=0)
    with pytest.raises(ValueError, match="target_under_score > 0 needs `neighbors`"):
        search(UntouchableLayout(), neighbors=None)
    with pytest.raises(ValueError, match="neighbor_alpha must be finite"):
        search(UntouchableLayout(), neighbor_alpha=np.nan)
    with pytest.raises(ValueError, match="cbv_correct_optimized needs flux errors"):
        search(UntouchableLayout(flux_errors=False))
    with pytest.raises(AssertionError, match="asked for prepare"):          # with sound arguments the layout is asked next
        search(UntouchableLayout())


def test_a_metric_layout_uploads_on_the_stream_of_the_batch_whose_kernel_reads(monkeypatch):
    """``over_fitting_metric`` builds its layout on the ORIGINAL batch and launches on the corrected one's stream: the kept
    cadences must be queued there too, or nothing orders the kernel after the copy."""
    seen = []

    def upload(handle, host, stream, dtype=np.float64):
        seen.append((handle, stream, np.asarray(host).tolist()))
        return "buffer %d" % len(seen), host

    monkeypatch.setattr(cotrend, "_upload", upload)

    class Batch(object):
        n_off, d_flux_err = np.array([0, 5, 10]), object()

        def __init__(self, handle, stream):
            self.handle, self.stream = handle, stream

        def __len__(self):
            return 2

    original, corrected = Batch("handle", 11), Batch("handle", 22)
    uniform = cotrend._UniformLayout(original, "over_fitting_metric", checked=(5, np.array([0, 2, 4], dtype=np.int32), 3, None))
    uniform.upload(corrected)
    rows = cotrend._RowsLayout(original, "over_fitting_metric",
                               checked=(np.array([0, 1, 2, 0, 1, 3], dtype=np.int32), np.array([0, 3, 6]), None))
    rows.upload(corrected)
    assert seen == [("handle", 22, [0, 2, 4]), ("handle", 22, [0, 1, 2, 0, 1, 3])]
    assert uniform.d_keep == "buffer 1" and rows.d_keep == "buffer 2" and len(uniform.keep) == len(rows.keep) == 1
    uniform.upload(corrected), rows.upload(corrected)           # resident once
    assert len(seen) == 2
