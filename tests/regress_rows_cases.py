"""Inputs shared by test_regress_rows_gpu.py and test_regress_rows_cpu.py: the generated batches of test_regress_shared_gpu.py
(``make_shared``, restated here: existing test files are not imported for their helpers), made ragged, and the oracle's answer
per target on ``X[rows_b]``, computed once and handed out read-only.

Raggedness comes from ``default_rng(seed + 1000)``.  Every fifth target (b % 5 == 0) keeps all rows; every other target drops
the rows where ``rng.random(N) < 0.03`` and then one gap of N // 40 rows starting at ``rng.integers(0, N - N // 40 + 1)``;
target 1 also loses its first N // 3 rows (whole leading slices of the row axis are absent), target 2 its last N // 3.

``clip_margin`` replays the oracle's clip loop and returns how close, in standard deviations of the pass, any residual of any
inner pass of any iteration comes to a clip bound.  ``problem`` asserts margin > 1e-3 sd for every target before it hands
anything out, so a changed generator cannot hide a flipped mask behind a tolerance."""
import numpy as np

from oracle import np_oracle as O

CONFIGS = [(11, 37, 1003, 17), (12, 19, 517, 3), (13, 21, 2050, 33), (14, 17, 700, 64)]
MIN_MARGIN_SD = 1e-3


def make_shared(seed, B, N, K, noutl=6):
    t = np.linspace(0, 30, N)
    rng = np.random.default_rng(seed)
    cols = [np.sin(2 * np.pi * t * rng.uniform(0.05, 3.0) + rng.uniform(0, 6)) for _ in range(K - 1)]
    X = np.column_stack(cols + [np.ones(N)])
    W = rng.normal(0, 1e-3, (B, K))
    W[:, -1] = 1.0
    err = rng.uniform(0.5, 2.0, (B, N)) * 2e-4
    y = W @ X.T + rng.normal(0, 1, (B, N)) * err
    cm = np.ones((B, N), bool)
    for b in range(B):
        y[b, rng.integers(0, N, noutl)] += rng.choice([-1, 1], noutl) * 0.01
        lo = int(rng.integers(0, N - N // 50 + 1))
        cm[b, lo:lo + N // 50] = False
    return X, y, err, cm


def ragged_rows(seed, B, N):
    """rows_b (ascending indices into the N grid rows) for every target."""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for b in range(B):
        keep = np.ones(N, bool)
        if b % 5 != 0:
            keep &= ~(rng.random(N) < 0.03)
            lo = int(rng.integers(0, N - N // 40 + 1))
            keep[lo:lo + N // 40] = False
        if b == 1:
            keep[:N // 3] = False
        if b == 2:
            keep[N - N // 3:] = False
        out.append(np.flatnonzero(keep).astype(np.int32))
    return out


def clip_margin(X, y, err, cm=None, prior_mu=None, prior_sigma=None, sigma=5.0, niters=5):
    """The oracle's loop (np_oracle.regression_correct / sigma_clip_mask) with a ruler: min over iterations, inner passes and
    residuals of |r - bound| / std."""
    n = len(y)
    err = np.ones(n) if err is None else err
    cm = np.ones(n, bool) if cm is None else cm
    outl = np.zeros(n, bool)
    margin = np.inf
    for _ in range(niters):
        m = cm & ~outl
        Xm = X[m]
        A = Xm.T.dot(Xm / err[m, None] ** 2)
        Bv = np.dot(Xm.T, y[m] / err[m] ** 2)
        if prior_sigma is not None:
            A = A + np.diag(1.0 / prior_sigma ** 2)
            Bv = Bv + prior_mu / prior_sigma ** 2
        r = y - X.dot(np.linalg.solve(A, Bv))
        d = r
        nchanged, it = 1, 0
        lo, hi = -np.inf, np.inf
        while nchanged != 0 and it < 5:
            it += 1
            size = d.size
            cen, std = np.median(d), np.std(d)
            lo, hi = cen - std * sigma, cen + std * sigma
            margin = min(margin, np.min(np.minimum(np.abs(r - lo), np.abs(r - hi))) / std)
            d = d[(d >= lo) & (d <= hi)]
            nchanged = size - d.size
        outl |= (r < lo) | (r > hi)
    return margin


class Ragged(object):
    """One generated ragged batch: the grid matrix X (N, K), rows per target, the packed arrays and their offsets."""

    def __init__(self, seed, B, N, K):
        self.seed, self.B, self.N, self.K = seed, B, N, K
        self.X, self.y2, self.err2, self.cm2 = make_shared(seed, B, N, K)
        self.rows_b = ragged_rows(seed, B, N)
        self.n_off = np.concatenate([[0], np.cumsum([len(r) for r in self.rows_b])]).astype(np.int64)
        self.rows = np.concatenate(self.rows_b)
        self.y = np.concatenate([self.y2[b, r] for b, r in enumerate(self.rows_b)])
        self.err = np.concatenate([self.err2[b, r] for b, r in enumerate(self.rows_b)])
        self.cm = np.concatenate([self.cm2[b, r] for b, r in enumerate(self.rows_b)])
        for a in (self.X, self.y2, self.err2, self.cm2, self.n_off, self.rows, self.y, self.err, self.cm):
            a.setflags(write=False)

    def sl(self, b):
        return slice(int(self.n_off[b]), int(self.n_off[b + 1]))

    def refs(self, with_err=True, with_mask=True, mu=None, sg=None):
        """The oracle per target on X[rows_b]; the clip margin of every target is asserted first."""
        out = []
        for b, r in enumerate(self.rows_b):
            s = self.sl(b)
            e = self.err[s] if with_err else None
            c = self.cm[s] if with_mask else None
            pm, ps = (None, None) if mu is None else (mu[b], sg[b])
            margin = clip_margin(self.X[r], self.y[s], e, c, pm, ps)
            assert margin > MIN_MARGIN_SD, ("a residual sits %.2e sd from a clip bound" % margin, self.seed, b)
            out.append(O.regression_correct(self.X[r], self.y[s], e, c, pm, ps))
        return out


_CACHE = {}


def problem(seed, B, N, K):
    """(Ragged, oracle answers with errors and mask), made once per configuration."""
    key = (seed, B, N, K)
    if key not in _CACHE:
        rg = Ragged(seed, B, N, K)
        _CACHE[key] = (rg, rg.refs())
    return _CACHE[key]


def check(r, rg, refs, targets=None):
    """The house tolerances of test_regress_shared_gpu.py on packed results: masks identical, model within 1e-9 std(y_b),
    coefficients rtol 1e-6 / atol 1e-9."""
    targets = range(rg.B) if targets is None else targets
    for b, ref in zip(targets, refs):
        s = rg.sl(b)
        assert np.array_equal(r["outlier_mask"][s], ref["outlier_mask"]), b
        dev = np.max(np.abs(r["model"][s] - ref["model"])) / np.std(rg.y[s])
        assert dev < 1e-9, (b, dev)
        assert np.allclose(r["coefficients"][b], ref["coefficients"], rtol=1e-6, atol=1e-9), b
