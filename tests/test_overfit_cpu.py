"""No GPU: the numpy restatement of the device noise generator against the Random123 known answers, the closed form
overfit.hip implements against the oracle's ``overfit_metric_lombscargle``, the declarations, and the argument checks that come
before any device call."""
import os
import re

import numpy as np
import pytest

import overfit_cases as C
from lightkurve_amd import _capi
from lightkurve_amd import device as D
from lightkurve_amd.correctors import metrics
from oracle import np_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every cadence count the GPU parity tests use, and the three the fields were measured at
PARITY_N = (5, 63, 64, 65, 127, 128, 129, 257)
CPU_N = (64, 257, 1000)


def oracle_ls(t, rows, frequency):
    return np.array([O.lk_ls_periodogram(t, r, frequency, exact=False) for r in rows])


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(np.atleast_1d(x)[0]) for x in C.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, key)
    # as arrays: the same words as one call per element
    i = np.arange(7)
    arr = C.philox4x32_10(i, 3, 2, 1, 5, 6)
    for j in i:
        assert tuple(int(x[j]) for x in arr) == tuple(int(np.atleast_1d(x)[0]) for x in C.philox4x32_10(int(j), 3, 2, 1, 5, 6))


def test_mirror_normals_are_standard_normal_and_counter_addressed():
    z = C.normals(200001, 0, 0)
    assert z.shape == (200001,) and np.all(np.isfinite(z)) and np.abs(z).max() <= 8.6
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.std() - 1) < 5 / np.sqrt(2 * z.size)
    q = np.sort(z)
    from math import erf
    cdf = 0.5 * (1 + np.vectorize(erf)(q[::100] / np.sqrt(2)))
    assert np.max(np.abs(cdf - (np.arange(q.size)[::100] + 0.5) / q.size)) < 1.95 / np.sqrt(z.size)      # KS at p ~ 0.001
    # an odd count drops the second value of the last pair and changes nothing else; every coordinate of the counter matters
    assert np.array_equal(C.normals(9, 1, 2, 3, 4), C.normals(10, 1, 2, 3, 4)[:9])
    base = C.normals(10, 1, 2, 3, 4)
    for other in (C.normals(10, 0, 2, 3, 4), C.normals(10, 1, 3, 3, 4), C.normals(10, 1, 2, 5, 4), C.normals(10, 1, 2, 3, 0),
                  C.normals(10, 1, 2, 3 + (1 << 32), 4)):
        assert not np.any(other == base)
    r = C.RandnFromMirror(3, seed=9, first_target=4, stream_id=2)
    got = [r(6, 1) for _ in range(4)]
    assert got[0].shape == (6, 1) and np.array_equal(got[3][:, 0], C.normals(6, 0, 5, 9, 2))
    assert np.array_equal(got[2][:, 0], C.normals(6, 2, 4, 9, 2))


@pytest.mark.parametrize("N", sorted(set(PARITY_N + CPU_N)))
def test_no_change_value_of_a_field_sits_at_zero(N):
    """n_up is a count: a ``change`` value that rounds across zero would move the metric by about 1 / n_up.  Every field the
    parity tests use keeps min |change| above 1e-9 max(P0, P1) (the LS routes agree to 1e-10 or better); variant ``a`` is the
    original itself: the same bits, change exactly zero on every route."""
    f = C.field(N)
    worst = np.inf
    for name in C.VARIANTS:
        metric, margin = C.closed_form(oracle_ls, f["t"], f["y"], f["variants"][name], f["err"], 1)
        if name == "a":
            assert np.all(np.isinf(margin)) and np.all(metric == 1.0)
        else:
            worst = min(worst, margin.min())
    print("N = %d: min |change| / max(P0, P1) = %.2e" % (N, worst))
    assert worst > 1e-9


@pytest.mark.parametrize("N", CPU_N)
@pytest.mark.parametrize("n_samples", [1, 3])
def test_closed_form_equals_the_oracle_metric(N, n_samples, monkeypatch):
    """Same spectra (the oracle's 'fast' periodogram) and same noise (numpy.random.randn replaced by the mirror's normals in
    call order): only the order of the sums differs."""
    f = C.field(N)
    B = f["y"].shape[0]
    worst, span = 0.0, []
    for name in C.VARIANTS:
        got, _ = C.closed_form(oracle_ls, f["t"], f["y"], f["variants"][name], f["err"], n_samples, seed=7, first_target=3, stream_id=1)
        monkeypatch.setattr(np.random, "randn", C.RandnFromMirror(n_samples, seed=7, first_target=3, stream_id=1))
        ref = np.array([O.overfit_metric_lombscargle(f["t"], f["y"][b], f["err"][b], f["variants"][name][b], f["err"][b], n_samples)
                        for b in range(B)])
        assert np.random.randn.calls == B * n_samples
        worst = max(worst, float(np.max(np.abs(got - ref))))
        span.append(float(np.median(ref)))
    print("N = %d, n_samples = %d: max |closed form - oracle| = %.2e; medians by variant %s"
          % (N, n_samples, worst, " ".join("%.3f" % s for s in span)))
    assert worst < 1e-9
    # the fields span the metric's range: the original exactly 1, a good fit in the upper half, then falling with the injected
    # noise to near the bottom at four times the uncertainty
    assert span[0] == 1.0 and span[1] > 0.5 and span[1] > span[2] > span[3] > span[4] > span[5] and span[5] < 0.15


def test_entry_points_are_declared_with_the_arguments_the_header_lists():
    text = open(os.path.join(ROOT, "include", "lkhip.h")).read()
    assert "metrics.py:24-138" in text and "(i, k, first_target + b, stream_id)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lk_[a-z0-9_]+)\s*\(", code))
    table = {s[0]: s for s in _capi.SIGNATURES}
    want = {"lk_overfit_metric_batch": 18, "lk_overfit_metric_batch_dev": 20, "lk_overfit_scratch_bytes": 7, "lk_overfit_noise_batch_dev": 9}
    for name, nargs in want.items():
        assert name in declared and name in table, name
        assert len(table[name][2]) == nargs, name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1)
        assert len(decl.split(",")) == nargs, name
    assert "overfit_metric_batch" in metrics.__all__


def test_argument_checks_need_no_device():
    keep, n, grid = _capi.overfit_arguments(30)
    assert keep is None and n == 30 and grid is None
    cm = np.zeros(30, dtype=bool)
    cm[[3, 4, 20]] = True
    keep, n, grid = _capi.overfit_arguments(30, cadence_mask=cm, frequency=0.5 + 0.25 * np.arange(4))
    assert keep.dtype == np.int32 and list(keep) == [3, 4, 20] and n == 3 and grid == (0.5, 0.25, 4)
    t, y = np.arange(30.0), np.ones((4, 30))
    for call in (lambda **k: _capi.overfit_metric_batch(t, y, y, y, **k), lambda **k: metrics.overfit_metric_batch(t, y, y, y, **k)):
        with pytest.raises(ValueError, match="n_samples must be >= 1"):
            call(n_samples=0)
        with pytest.raises(ValueError, match=r"shape \(30,\)"):
            call(cadence_mask=np.ones(29, dtype=bool))
        with pytest.raises(ValueError, match=r"shape \(30,\)"):
            call(cadence_mask=np.ones((4, 30), dtype=bool))
        two = np.zeros(30, dtype=bool)
        two[[7, 9]] = True
        with pytest.raises(ValueError, match="at least three kept cadences"):
            call(cadence_mask=two)
        with pytest.raises(ValueError, match="at least two frequencies"):
            call(frequency=[1.0])
        with pytest.raises(ValueError, match="regular"):
            call(frequency=[1.0, 2.0, 4.0])
        with pytest.raises(ValueError, match="regular"):
            call(frequency=[3.0, 2.0, 1.0])
        with pytest.raises(ValueError, match="seed"):
            call(seed=-1)
        with pytest.raises(ValueError, match="32 bits"):
            call(first_target=(1 << 32) - 3)
        with pytest.raises(ValueError, match="stream_id"):
            call(stream_id=1 << 32)
    bad = y.copy()
    bad[2, 5] = np.nan
    with pytest.raises(ValueError, match="remove_nans"):
        _capi.overfit_metric_batch(t, y, bad, y)
    with pytest.raises(ValueError, match="remove_nans"):
        _capi.overfit_metric_batch(t, bad, y, y)
    with pytest.raises(ValueError, match="B >= 1"):
        _capi.overfit_metric_batch(t, np.ones(30), np.ones(30), np.ones(30))
    with pytest.raises(ValueError, match="one shape"):
        _capi.overfit_metric_batch(t, y, np.ones((4, 29)), y)
    with pytest.raises(ValueError, match="flux errors"):
        _capi.overfit_metric_batch(t, y, y, None)
    with pytest.raises(ValueError, match=r"time must be"):
        _capi.overfit_metric_batch(np.arange(29.0), y, y, y)


def test_scratch_plan_needs_no_device():
    """The block holds z0, z1, and per round of R samples the times, the noise rows and their spectra, plus P0 and P1."""
    B, n, M, ns = 1000, 20000, 50000, 10
    rows, spec = B * n * 8, B * M * 8
    full, r_full = _capi.overfit_scratch_bytes(B, n, M, ns, 1 << 40)
    assert r_full == ns and 2 * rows + 2 * spec + ns * (2 * rows + spec) <= full < 2 * rows + 2 * spec + ns * (2 * rows + spec) + (1 << 20)
    dflt, r_dflt = _capi.overfit_scratch_bytes(B, n, M, ns)
    assert dflt <= _capi.OVERFIT_SCRATCH_DEFAULT and 1 <= r_dflt < ns
    assert _capi.overfit_scratch_bytes(B, n, M, ns, dflt) == (dflt, r_dflt)          # the size it returns buys the same rounds
    one, r_one = _capi.overfit_scratch_bytes(B, n, M, ns, 1)                          # nothing fits: one sample per round
    assert r_one == 1 and one < dflt
    for bad in ((0, n, M, ns), (B, 2, M, ns), (B, n, 1, ns), (B, n, M, 0)):
        with pytest.raises(ValueError):
            _capi.overfit_scratch_bytes(*bad)


def _batch_without_a_device(n_off, nan_free, err=True):
    """A DeviceLightCurveBatch with offsets only: enough for the checks that run before the first device call."""
    b = object.__new__(D.DeviceLightCurveBatch)
    b.n_off = np.asarray(n_off, dtype=np.int64)
    b.nan_free = nan_free
    b.d_flux_err = object() if err else None
    return b


def test_resident_method_checks_come_before_any_device_call():
    ok = _batch_without_a_device([0, 100, 200], True)
    with pytest.raises(ValueError, match="between 90 and 100 cadences"):
        _batch_without_a_device([0, 100, 190], True).over_fitting_metric(ok)
    with pytest.raises(ValueError, match="between 90 and 100 cadences"):
        ok.over_fitting_metric(_batch_without_a_device([0, 100, 190], True))
    with pytest.raises(ValueError, match=r"remove_nans\(\)"):
        _batch_without_a_device([0, 100, 200], False).over_fitting_metric(ok)
    with pytest.raises(ValueError, match=r"remove_nans\(\)"):
        ok.over_fitting_metric(_batch_without_a_device([0, 100, 200], False))
    with pytest.raises(ValueError, match=r"\(2 x 100\)"):
        ok.over_fitting_metric(_batch_without_a_device([0, 100, 200, 300], True))
    with pytest.raises(ValueError, match=r"\(2 x 100\)"):
        ok.over_fitting_metric(_batch_without_a_device([0, 99, 198], True))
    with pytest.raises(ValueError, match="resident batch"):
        ok.over_fitting_metric(np.ones((2, 100)))
    with pytest.raises(ValueError, match="flux errors"):
        _batch_without_a_device([0, 100, 200], True, err=False).over_fitting_metric(ok)
    with pytest.raises(ValueError, match="n_samples must be >= 1"):
        ok.over_fitting_metric(ok, n_samples=0)
    with pytest.raises(ValueError, match="at least two frequencies"):
        ok.over_fitting_metric(ok, frequency=[0.5])
    with pytest.raises(ValueError, match="regular"):
        ok.over_fitting_metric(ok, frequency=[0.5, 1.0, 2.5])
    with pytest.raises(ValueError, match=r"shape \(100,\)"):
        ok.over_fitting_metric(ok, cadence_mask=np.ones(99, dtype=bool))
    two = np.zeros(100, dtype=bool)
    two[:2] = True
    with pytest.raises(ValueError, match="at least three kept cadences"):
        ok.over_fitting_metric(ok, cadence_mask=two)
    with pytest.raises(ValueError, match="at least three kept cadences"):
        ok.cbv_goodness_scan(np.ones((100, 2)), [1.0], cadence_mask=two)
