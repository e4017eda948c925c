"""GPU parity: the WIDE family of regress_launch against the numpy oracle.  The solver changes at K = 141 / 142 (the augmented
system of solve_lds_kernel needs K (K + 1) + 2 K + 34 doubles of the 160 KB = 20480 an LDS plan has: 20338 at K = 141, 20624
at K = 142, where the global-memory LU solve_kernel takes over), the Gram kernel at K + 1 = 144 / 145 columns (gram_tri_kernel
-> the 64 x 64-block gram_mfma_kernel), and invert_kernel has no LDS form at any width.  test_regress_gpu.py presses on the
narrow side; this file presses on the other one: priors in solve_kernel, the covariance above K = 141, the delta Gram over
several block pairs and its list overflow, per-target convergence in a ragged batch, a NaN column on the global pivot search,
run-to-run bits.

Bars (those of test_regress_gpu.py): outlier masks identical; max |model - ref| < 1e-9 std(y); coefficients rtol 1e-6, atol
1e-9; covariance within 1e-8 of sqrt(outer(diag, diag)) and symmetric to 1e-12 of its largest entry.  The white regressors of
make_problem(smooth=False) keep the systems well posed (condition numbers 15 .. 2.5e3 with N >= K + 58; there the float64
oracle is itself within 5e-12 std(y) of a long-double elimination).  No target has N < K: with priors alone holding the
system up its condition number is 5e7 and the oracle is 1.2e-7 std(y) from the long-double solve — the bar would measure
the reference.

Every comparison prints its figure before it asserts (pytest -s / -rP shows them)."""
import functools

import numpy as np
import pytest

from lightkurve_amd import _capi
from oracle import np_oracle as O
from tests.test_determinism_gpu import _disturb, thrice
from tests.test_regress_gpu import make_problem

pytestmark = pytest.mark.gpu


def half_priors(rng, B, K):
    """prior_mu of size 1e-3 (not zero: a dropped mu / sigma^2 term moves the model by about 1e-7 std(y), a hundred bars),
    prior_sigma 0.05 on every second column and none (inf) on the rest."""
    mu = rng.normal(0, 1e-3, (B, K))
    sg = np.full((B, K), np.inf)
    sg[:, ::2] = 0.05
    return mu, sg


def batch(problems):
    Xs, ys, es, cms = zip(*problems)
    off = np.r_[0, np.cumsum([len(y) for y in ys])]
    return np.vstack(Xs), np.concatenate(ys), off, np.concatenate(es), np.concatenate(cms)


def check_target(tag, r, off, b, y, ref, model_bar=1e-9, coefficients=True):
    s = slice(off[b], off[b + 1])
    dm = np.max(np.abs(r["model"][s] - ref["model"])) / np.std(y)
    dw = np.max(np.abs(r["coefficients"][b] - ref["coefficients"]) / (1e-9 + 1e-6 * np.abs(ref["coefficients"])))
    print("%s target %d: %d outliers, model %.2e std(y), coefficients %.2e of their bar" % (tag, b, ref["outlier_mask"].sum(), dm, dw))
    assert np.array_equal(r["outlier_mask"][s], ref["outlier_mask"]), (tag, b)
    assert dm < model_bar, (tag, b)
    if coefficients:
        assert np.allclose(r["coefficients"][b], ref["coefficients"], rtol=1e-6, atol=1e-9), (tag, b)


def check_cov(tag, cov, ref):
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    d = np.max(np.abs(cov - ref) / scale)
    asym = np.max(np.abs(cov - cov.T)) / np.max(np.abs(cov))
    print("%s covariance: %.2e of sqrt(outer(diag, diag)), asymmetry %.2e of the largest entry" % (tag, d, asym))
    assert d < 1e-8, tag
    assert np.allclose(cov, cov.T, rtol=0, atol=1e-12 * np.max(np.abs(cov))), tag


@pytest.mark.parametrize("K", [141, 142, 143, 144, 145, 192, 193, 257])
def test_both_sides_of_every_route_boundary_with_priors(K):
    """141 | 142: the last LDS solve and the first global one; 143 | 144: the last narrow Gram and the first block Gram
    (K + 1 = 144 | 145 columns); 192 | 193: KB = 3 -> 4 blocks of 64 for [X | y]; 257: a second trip of model_kernel's
    256-column loop.  Ragged N (several 32-cadence stages, a partial last one), errors, a cadence mask, priors on every
    second column, 8 outliers per target so that passes 2.. subtract a short list over every block pair (the short target
    keeps most of its own: it is done after the first pass while its neighbours go on).
    Measured: models within 3.0e-12 std(y) (the short target; 1.1e-12 on the long ones), coefficients within 4e-6 of their bar."""
    rng = np.random.default_rng(1000 + K)
    ns = [K + 60, 600, 517]
    probs = [make_problem(rng, n, K, 8, smooth=False) for n in ns]
    X, y, off, err, cm = batch(probs)
    mu, sg = half_priors(rng, len(ns), K)
    r = _capi.regress_batch(X, y, off, err=err, cadence_mask=cm, prior_mu=mu, prior_sigma=sg)
    refs = [O.regression_correct(Xb, yb, eb, cb, mu[b], sg[b]) for b, (Xb, yb, eb, cb) in enumerate(probs)]
    # (the fit of the short target, 60 cadences more than columns, soaks up most of its outliers; the two long ones lose theirs)
    assert refs[1]["outlier_mask"].sum() >= 5 and refs[2]["outlier_mask"].sum() >= 5
    for b, p in enumerate(probs):
        check_target("K=%d" % K, r, off, b, p[1], refs[b])


def test_full_width_k465_with_priors_normal_equations_and_covariance():
    """K = 465, the width of a PLD design matrix at 20 000 cadences, with the priors such a matrix carries: the fit the
    kernels return solves the normal equations of the LAST pass, X^T W (y - X w) + (mu - w) / sigma^2 = 0 per column to 1e-9
    of |X|^T W |y| + |mu| / sigma^2 (test_full_width_k465_properties with the prior terms; the mask of the last fit is the
    outlier set after niters - 1 passes, taken from the oracle, whose masks the kernels must reproduce).  Masks and model
    against the oracle at that test's 1e-8 std(y); the 465 x 465 Gauss-Jordan inverse against the oracle's np.linalg.inv.
    Measured: gradient 2.2e-15, model 4.6e-13 std(y), covariance 8.5e-15, asymmetry 3.2e-16."""
    rng = np.random.default_rng(465)
    n, K = 1500, 465
    X, y, err, cm = make_problem(rng, n, K, 20, smooth=False)
    mu, sg = half_priors(rng, 1, K)
    r = _capi.regress_batch(X, y, [0, n], err=err, cadence_mask=cm, prior_mu=mu, prior_sigma=sg, return_cov=True)
    ref = O.regression_correct(X, y, err, cm, mu[0], sg[0])
    check_target("K=465", r, [0, n], 0, y, ref, model_bar=1e-8, coefficients=False)
    m = cm & ~O.regression_correct(X, y, err, cm, mu[0], sg[0], niters=4)["outlier_mask"]
    w = r["coefficients"][0]
    grad = X[m].T @ ((y[m] - X[m] @ w) / err[m] ** 2) + (mu[0] - w) / sg[0] ** 2
    scale = np.abs(X[m].T) @ (np.abs(y[m]) / err[m] ** 2) + np.abs(mu[0]) / sg[0] ** 2
    print("K=465 normal equations: %.2e" % np.max(np.abs(grad) / scale))
    assert np.max(np.abs(grad) / scale) < 1e-9
    check_cov("K=465", r["coefficients_cov"][0], ref["coefficients_cov"])


@pytest.mark.parametrize("K", [142, 200])
def test_covariance_on_the_wide_path_vs_oracle(K):
    """invert_kernel paired with the global solve (K = 135 in test_covariance_batch_k135_vs_oracle sits on the LDS one), 3 and
    4 blocks of 64.  Finite priors on all columns, and tight enough to count: sigma = 1e-3 — the size of the coefficients —
    puts 1 / sigma^2 = 1e6 on a diagonal of about N / err^2 = 2e10, 5e-5 of it, so an inverse without the prior term is
    5e3 bars away (at the sigma = 10 of the K = 135 test it would be 1e-12 and pass).  The constant column, whose coefficient
    is 1, keeps a wide prior.  Measured: covariance within 5.2e-15, asymmetry 2.6e-16, models within 6.8e-13 std(y)."""
    rng = np.random.default_rng(7000 + K)
    probs = [make_problem(rng, n, K, 10, smooth=False) for n in (700, 1100)]
    X, y, off, err, cm = batch(probs)
    mu = rng.normal(0, 1e-3, (2, K))
    sg = np.full((2, K), 1e-3)
    sg[:, -1] = 10.0
    r = _capi.regress_batch(X, y, off, err=err, cadence_mask=cm, prior_mu=mu, prior_sigma=sg, return_cov=True)
    for b, (Xb, yb, eb, cb) in enumerate(probs):
        ref = O.regression_correct(Xb, yb, eb, cb, mu[b], sg[b])
        check_target("cov K=%d" % K, r, off, b, yb, ref)
        check_cov("cov K=%d target %d" % (K, b), r["coefficients_cov"][b], ref["coefficients_cov"])


@functools.lru_cache(maxsize=None)
def overflow_problem():
    """K = 150 (3 blocks of 64: six block pairs), three targets: 280 outliers of one amplitude in 8000 cadences (3.5 % at
    5.4 sigma of the first residual: the first clip takes them all at once, more than the 256 the list holds); three tiers
    of 40 in 3000 (the small ones only stand out once the large ones are gone: several passes of short lists); none in
    2500 (done after pass 1 while its neighbours go on).  Returns (call arguments, problems, references); treat as read-only."""
    K = 150
    ns = [8000, 3000, 2500]
    rng = np.random.default_rng(5)
    p0 = make_problem(rng, ns[0], K, 0, smooth=False)
    p0[1][rng.choice(ns[0], 280, replace=False)] += 1.0
    rng = np.random.default_rng(6)
    p1 = make_problem(rng, ns[1], K, 0, smooth=False)
    for amp, cnt in ((0.5, 40), (0.02, 40), (0.004, 40)):
        p1[1][rng.choice(ns[1], cnt, replace=False)] += amp * rng.choice([-1, 1], cnt)
    p2 = make_problem(rng, ns[2], K, 0, smooth=False)
    probs = (p0, p1, p2)
    X, y, off, err, cm = batch(probs)
    mu, sg = half_priors(rng, 3, K)
    refs = [[O.regression_correct(Xb, yb, eb, cb, mu[b], sg[b], niters=it) for it in (1, 2, 3, 5)]
            for b, (Xb, yb, eb, cb) in enumerate(probs)]
    return dict(X=X, y=y, n_off=off, err=err, cadence_mask=cm, prior_mu=mu, prior_sigma=sg), probs, refs


def test_list_overflow_on_several_blocks_and_mixed_convergence_vs_oracle():
    """The delta Gram over six block pairs: a target whose 256-entry list overflows (recomputed in full, the other targets'
    lists in the same launch), a target that takes several passes of short lists, and one that is done after the first pass
    and must be left alone by every later kernel.  The reference says that the cases are what they are said to be.
    Measured: 280 / 282 / 282 outliers after 1 / 2 / 5 passes, 40 / 80 / 119 / 119, none; models within 3.7e-13 std(y)."""
    args, probs, refs = overflow_problem()
    r = _capi.regress_batch(args["X"], args["y"], args["n_off"], **{k: args[k] for k in ("err", "cadence_mask", "prior_mu", "prior_sigma")})
    counts = [[int(ref["outlier_mask"].sum()) for ref in per] for per in refs]      # after 1, 2, 3 and 5 passes
    print("outliers after 1, 2, 3, 5 passes:", counts)
    assert counts[0][0] > 256 and counts[0][3] >= 280                              # one clip overflows the list
    assert 0 < counts[1][0] <= 256 and 0 < counts[1][1] - counts[1][0] <= 256      # short lists, pass after pass
    assert 0 < counts[1][2] - counts[1][1] <= 256 and counts[1][3] >= 100
    assert counts[2] == [0, 0, 0, 0]                                               # converged at once
    for b, p in enumerate(probs):
        check_target("overflow", r, args["n_off"], b, p[1], refs[b][3])


@pytest.mark.parametrize("niters", [1, 2])
def test_one_and_two_passes_at_k145(niters):
    """niters = 1: the full block Gram only; niters = 2: exactly one delta pass on top of it.
    Measured: models within 1.2e-12 std(y)."""
    K = 145
    rng = np.random.default_rng(145)
    ns = [K + 60, 600, 517]
    probs = [make_problem(rng, n, K, 8, smooth=False) for n in ns]
    X, y, off, err, cm = batch(probs)
    mu, sg = half_priors(rng, len(ns), K)
    r = _capi.regress_batch(X, y, off, err=err, cadence_mask=cm, prior_mu=mu, prior_sigma=sg, niters=niters)
    refs = [O.regression_correct(Xb, yb, eb, cb, mu[b], sg[b], niters=niters) for b, (Xb, yb, eb, cb) in enumerate(probs)]
    assert refs[1]["outlier_mask"].sum() >= 5 and refs[2]["outlier_mask"].sum() >= 5
    for b, p in enumerate(probs):
        check_target("niters=%d" % niters, r, off, b, p[1], refs[b])


def test_nan_column_on_the_global_solver_gives_nan_coefficients():
    """test_nan_regressor_column_gives_nan_coefficients_not_a_fault for solve_kernel: its pivot search starts every thread
    at row j and never takes a NaN candidate, so the pivot row stays in range; the coefficients of the target with the NaN
    column are all NaN, as numpy.linalg.solve's are, and the other target of the batch equals the oracle (measured: model within
    6.5e-13 std(y))."""
    rng = np.random.default_rng(150)
    K, ns = 150, [600, 450]
    probs = [make_problem(rng, n, K, 4, smooth=False) for n in ns]
    probs[0][0][:, 5] = np.nan
    X, y, off, err, cm = batch(probs)
    r = _capi.regress_batch(X, y, off, err=err, cadence_mask=cm)
    assert np.all(np.isnan(r["coefficients"][0]))
    Xb, yb, eb, cb = probs[1]
    check_target("NaN column", r, off, 1, yb, O.regression_correct(Xb, yb, eb, cb))


def test_wide_batch_run_to_run_same_bits():
    """The K = 150 call above — overflow, short lists and an early finisher in one launch — twice, and once more after another
    entry point has used the device scratch: all outputs bitwise equal (the delta list is ascending whatever the scheduling,
    and the delta Gram sums over it in that order)."""
    args, _, _ = overflow_problem()
    thrice(lambda: _capi.regress_batch(args["X"], args["y"], args["n_off"], err=args["err"], cadence_mask=args["cadence_mask"],
                                       prior_mu=args["prior_mu"], prior_sigma=args["prior_sigma"], return_cov=True),
           _disturb, "wide regression")
