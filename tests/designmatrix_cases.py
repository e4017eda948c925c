"""Inputs and plain references behind tests/test_designmatrix_cases_cpu.py, tests/test_designmatrix_edges_gpu.py,
tests/test_savgol_design_cpu.py and the high-polyorder case of tests/test_flatten_gpu.py: lk_standardize_batch
(dm_standardize_kernel, regress.hip), lk_spline_basis_batch (bspline_row, spline_basis.hpp) and lk_savgol_design
(savgol_design, flatten.hip).  numpy and the standard library only.

  * standardize_reference: DesignMatrix.standardize as documented — zeros and NaN are missing, the median is the exact order
    statistic, the standard deviation is two-pass in np.longdouble and rounded once, a column whose kept values are all equal
    (min == max) is left unchanged.  numpy's own nanstd is NOT the yardstick on such columns: it is non-zero for 600 copies of
    0.1 and zero for 5 (tests/test_designmatrix_cases_cpu.py shows it), so the documented contract is.
  * bspline_reference: Cox-de Boor in fractions.Fraction on the exact values of the doubles, rounded once.
  * savgol_reference: the least-squares polynomial's hat matrix over integer abscissae in exact integer arithmetic, rounded
    once.

The references are cached per case (functools.lru_cache) and must be left unchanged by their users."""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

# ------------------------------------------------------------------------------------------------------ standardize


def column_kind(v):
    """'empty' (nothing kept), 'constant' (all kept values equal), 'nonfinite' (median or deviation not finite) or
    'toleranced' (everything else: compared within a tolerance) — the branch standardize_reference takes for the column."""
    v = np.asarray(v, dtype=np.float64)
    keep = ~np.isnan(v) & (v != 0)
    if not keep.any():
        return "empty"
    kv = v[keep]
    if kv.min() == kv.max():
        return "constant"
    return "toleranced" if np.all(np.isfinite(kv)) else "nonfinite"


def column_stats(v):
    """(median, mean, sd) of the kept values of a 'toleranced' or 'nonfinite' column: exact order statistic (mean of the two
    middle values for an even count, as np.nanmedian takes it), two-pass population deviation in longdouble rounded once."""
    v = np.asarray(v, dtype=np.float64)
    kv = np.sort(v[~np.isnan(v) & (v != 0)])
    n = kv.size
    with np.errstate(invalid="ignore", over="ignore"):
        med = kv[n // 2] if n % 2 else np.float64(kv[n // 2 - 1] + kv[n // 2]) / 2.0
        kl = kv.astype(np.longdouble)
        mean = kl.sum() / n
        sd = np.sqrt(((kl - mean) ** 2).sum() / n)
    return float(med), float(mean), float(sd)


def standardize_reference(A):
    """DesignMatrix.standardize of A (N, P) or (B, N, P), column by column.

    A column with a +-inf value has no finite median or deviation and comes back as zeros: the reading of the reference's last
    step (a fillna(0) over the whole frame) that the kernel comment's "missing values come back as 0" fits.  The reference's
    source is not at hand and the golden file holds no such column, so that reading is this file's, not a checked fact."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim == 3:
        return np.stack([standardize_reference(a) for a in A])
    out = np.zeros_like(A)
    for c in range(A.shape[1]):
        v = A[:, c]
        kind = column_kind(v)
        if kind == "constant":
            out[:, c] = np.where(np.isnan(v), 0.0, v)
        elif kind == "toleranced":
            keep = ~np.isnan(v) & (v != 0)
            med, _, sd = column_stats(v)
            out[keep, c] = (v[keep] - med) / sd
    return out


STD_N = (1, 2, 255, 256, 257, 600, 1000)
STD_P = (1, 13)
CONSTANTS = (0.1, 3.3, 1e-3)          # not representable: a rounded mean differs from the value


def _draws(rng, N, parity, with_nan):
    """Normal draws with ~5 % zeros (and ~5 % NaN), the kept count forced to the wanted parity; None if fewer than 2 are left."""
    v = 3.0 + 2.0 * rng.standard_normal(N)
    n_nan = (N + 19) // 20 if with_nan else 0
    n_zero = (N + 19) // 20
    if (N - n_nan - n_zero) % 2 != parity:
        n_zero += 1
    if N - n_nan - n_zero < 2:
        return None
    idx = rng.permutation(N)
    v[idx[:n_zero]] = 0.0
    v[idx[n_zero:n_zero + n_nan]] = np.nan
    return v


def _constant(value, variant):
    def build(rng, N):
        v = np.full(N, value)
        if variant == "zeros":
            v[1::2] = 0.0
        elif variant == "nan":
            v[2::3] = np.nan
        return v
    return build


def _one_kept(rng, N):
    v = np.where(np.arange(N) % 2 == 0, 0.0, np.nan)
    v[rng.integers(N)] = 0.7
    return v


def _two_equal(rng, N):
    if N < 2:
        return None
    v = np.where(np.arange(N) % 3 == 0, np.nan, 0.0)
    v[rng.choice(N, 2, replace=False)] = -1.3
    return v


def _offset(rng, N):
    if N < 2:
        return None
    z = rng.standard_normal(N)
    return 1e6 + 1.05 * (z - z.mean()) / z.std()      # unit scatter, scaled so that |mean| / sd stays under 1e6


def _neg_zero(rng, N):
    v = rng.standard_normal(N)
    v[::4] = -0.0
    return v


def _inf(both):
    def build(rng, N):
        if N < (3 if both else 2):
            return None
        v = rng.standard_normal(N)
        v[N // 2] = np.inf
        if both:
            v[0] = -np.inf
        return v
    return build


# name -> (builder(rng, N) -> column or None where N is too small for it, the kind expected at N >= 3)
FAMILIES = {
    "normal_odd": (lambda rng, N: _draws(rng, N, 1, False), "toleranced"),
    "normal_even": (lambda rng, N: _draws(rng, N, 0, False), "toleranced"),
    "nan_odd": (lambda rng, N: _draws(rng, N, 1, True), "toleranced"),
    "nan_even": (lambda rng, N: _draws(rng, N, 0, True), "toleranced"),
    "all_zero": (lambda rng, N: np.zeros(N), "empty"),
    "all_nan": (lambda rng, N: np.full(N, np.nan), "empty"),
    "one_kept": (_one_kept, "constant"),
    "two_equal_kept": (_two_equal, "constant"),
    "const_2.5": (_constant(2.5, "plain"), "constant"),
    "offset_1e6": (_offset, "toleranced"),
    "neg_zero": (_neg_zero, "toleranced"),
    "pos_inf": (_inf(False), "nonfinite"),
    "both_inf": (_inf(True), "nonfinite"),
}
for _v in CONSTANTS:
    for _variant in ("plain", "zeros", "nan"):
        FAMILIES["const_%g_%s" % (_v, _variant)] = (_constant(_v, _variant), "constant")

StdCase = namedtuple("StdCase", "name N P families A")      # A: (2, N, P), A[1] = A[0][:, perm]


def _std_case(N, names, tag):
    rng = np.random.default_rng(1000 * N + len(names))
    cols, kept = [], []
    for nm in names:
        v = FAMILIES[nm][0](rng, N)
        if v is not None:
            cols.append(v)
            kept.append(nm)
    while len(names) > 1 and len(cols) < len(names):       # a small N cannot hold every family: fill up with constants
        cols.append(np.full(N, 2.5))
        kept.append("const_2.5")
    A0 = np.stack(cols, axis=1)
    perm = rng.permutation(len(kept))
    return StdCase("N%d_%s" % (N, tag), N, len(kept), tuple(kept), np.stack([A0, A0[:, perm]])), perm


@functools.lru_cache(maxsize=None)
def standardize_cases():
    """[(StdCase, perm, reference (2, N, P))]: per N two matrices of 13 columns that hold every family between them (a family
    that a small N cannot hold gives way to a 2.5 column, the second matrix is filled up with further normal draws), and every family alone."""
    names = list(FAMILIES)
    wide = [("wide_a", names[:13]), ("wide_b", names[13:] + ["normal_odd", "nan_even", "normal_even", "nan_odd"])]
    assert all(len(g) == 13 for _, g in wide)
    out = []
    for N in STD_N:
        for tag, group in wide + [(nm, [nm]) for nm in names]:
            if all(FAMILIES[nm][0](np.random.default_rng(0), N) is None for nm in group):
                continue
            case, perm = _std_case(N, group, tag)
            out.append((case, perm, standardize_reference(case.A)))
    return out


# ----------------------------------------------------------------------------------------------------------- spline


def full_knots(knots, degree):
    """[lo, interior ..., hi] -> the clamped knot vector with degree + 1 copies of each bound."""
    knots = np.asarray(knots, dtype=np.float64)
    return np.concatenate([[knots[0]] * degree, knots, [knots[-1]] * degree])


def bspline_span(x, T, degree):
    """mu with T[mu] <= x < T[mu + 1] (comparisons of doubles are exact); x == T[-1] belongs to the last non-empty span.  The
    row's non-zero columns are mu - degree .. mu."""
    T = np.asarray(T, dtype=np.float64)
    if x == T[-1]:
        return int(np.flatnonzero(T[:-1] < T[1:])[-1])
    return int(np.searchsorted(T, x, side="right")) - 1


def bspline_reference(x, knots_full, degree):
    """Clamped B-spline basis of x (N,) on knots_full = [lo, interior knots, hi] -> (N, n_inner + degree + 1): the Cox-de Boor
    recursion in Fraction on the exact values of the doubles, 0/0 := 0, half-open spans, x == hi in the last non-empty span."""
    Tf = full_knots(knots_full, degree)
    T = [Fraction(float(k)) for k in Tf]
    ncol = len(T) - degree - 1
    xu, inverse = np.unique(np.asarray(x, dtype=np.float64), return_inverse=True)
    out = np.zeros((len(xu), ncol))
    for n, xv in enumerate(xu):
        xf = Fraction(float(xv))
        B = {bspline_span(xv, Tf, degree): Fraction(1)}              # degree 0: the indicator of the span
        for k in range(1, degree + 1):
            nxt = {}
            for i in set(B) | {j - 1 for j in B}:
                s = Fraction(0)
                if i in B and T[i + k] != T[i]:
                    s += (xf - T[i]) / (T[i + k] - T[i]) * B[i]
                if i + 1 in B and T[i + k + 1] != T[i + 1]:
                    s += (T[i + k + 1] - xf) / (T[i + k + 1] - T[i + 1]) * B[i + 1]
                if s:
                    nxt[i] = s
            B = nxt
        for i, s in B.items():
            out[n, i] = float(s)
    return out[inverse]


SPL_N = (1, 255, 256, 257, 513)
SplCase = namedtuple("SplCase", "name degree x knots")      # knots: (B, n_inner + 2); x: (N,), shared by the B knot vectors


def _spline_x(rng, knots, N):
    """Unsorted x in [lo, hi]: lo, hi, every interior knot and its two neighbours in double, filled up from 40 uniform draws
    (repeated values keep the exact reference, which is computed once per distinct x, quick at every N)."""
    lo, hi = knots[0], knots[-1]
    inner = np.unique(knots[1:-1])
    special = np.concatenate([[hi, lo], inner, np.nextafter(inner, -np.inf), np.nextafter(inner, np.inf)])
    special = special[(special >= lo) & (special <= hi)]
    if N <= special.size:
        x = np.concatenate([special[2:], special[:2]])[:N]      # N = 1: an interior knot where there is one
    else:
        x = np.concatenate([special, rng.choice(rng.uniform(lo, hi, 40), N - special.size)])
    return rng.permutation(x)


def _plain_inner(rng, n_inner, lo, hi):
    return np.sort(rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), n_inner))


def _structured_knots(kind, degree, lo, hi):
    a, b, c = lo + (hi - lo) * np.array([0.21, 0.5, 0.83])
    if kind == "double":
        inner = [a, b, b, c]
    elif kind == "full_multiplicity":
        inner = [a] + [b] * (degree + 1) + [c]
    elif kind == "equals_lo":
        inner = [lo, a, b]
    elif kind == "equals_hi":
        inner = [a, b, hi]
    else:
        assert kind == "ulp_apart"
        inner = [a, b, np.nextafter(b, np.inf), c]
    return np.concatenate([[lo], inner, [hi]])


SPL_STRUCTURES = ("double", "full_multiplicity", "equals_lo", "equals_hi", "ulp_apart")


@functools.lru_cache(maxsize=None)
def spline_cases():
    """Every degree 0..7 with every n_inner in {0, 1, 6, 20} at N = 257 (two tiles of pld_spline_kernel); the tile edges N = 1,
    255, 256, 513 at degree 3 and 7; every knot structure at every degree; three knot vectors on one x."""
    lo, hi = -1.7, 4.1
    cases = []

    def add(name, degree, knots, N, seed):
        rng = np.random.default_rng(seed)
        knots = np.atleast_2d(knots)
        cases.append(SplCase(name, degree, _spline_x(rng, knots[0], N), knots))

    for degree in range(8):
        for n_inner in (0, 1, 6, 20):
            rng = np.random.default_rng(100 * degree + n_inner)
            add("d%d_k%d_N257" % (degree, n_inner), degree, np.r_[lo, _plain_inner(rng, n_inner, lo, hi), hi], 257, degree)
    for degree, n_inner in ((3, 6), (7, 20)):
        for N in (1, 255, 256, 513):
            rng = np.random.default_rng(N + degree)
            add("d%d_k%d_N%d" % (degree, n_inner, N), degree, np.r_[lo, _plain_inner(rng, n_inner, lo, hi), hi], N, N)
    for kind in SPL_STRUCTURES:
        for degree in range(8):
            add("%s_d%d" % (kind, degree), degree, _structured_knots(kind, degree, lo, hi), 255, 7 * degree)
    rng = np.random.default_rng(3)
    three = np.stack([np.r_[lo, _plain_inner(rng, 6, lo, hi), hi], _structured_knots("double", 3, lo, hi)[[0, 1, 2, 2, 3, 3, 4, 5]],
                      np.r_[lo, _plain_inner(rng, 6, lo, hi), hi]])
    add("three_knot_vectors_d3", 3, three, 257, 11)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def spline_reference_of(name):
    """(B, N, n_inner + degree + 1) reference of the named case, computed once."""
    case = next(c for c in spline_cases() if c.name == name)
    return np.stack([bspline_reference(case.x, k, case.degree) for k in case.knots])


# ---------------------------------------------------------------------------------------------------- Savitzky-Golay


def _int_inverse(M):
    """(adj, det) of a square matrix of Python ints with M^-1 = adj / det exactly: Gauss-Jordan in Fraction."""
    n = len(M)
    A = [[Fraction(v) for v in row] + [Fraction(int(i == j)) for j in range(n)] for i, row in enumerate(M)]
    for j in range(n):
        p = next(i for i in range(j, n) if A[i][j] != 0)
        A[j], A[p] = A[p], A[j]
        A[j] = [v / A[j][j] for v in A[j]]
        for i in range(n):
            if i != j and A[i][j] != 0:
                f = A[i][j]
                A[i] = [a - f * b for a, b in zip(A[i], A[j])]
    inv = [row[n:] for row in A]
    det = 1
    for row in inv:
        for v in row:
            det = det * v.denominator // _gcd(det, v.denominator)
    return [[int(v * det) for v in row] for row in inv], det


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def savgol_reference(window, polyorder, rows=None):
    """(taps[w], edge[2, w // 2, w]) of the Savitzky-Golay design in the layout lk_savgol_design documents, exact and rounded
    once.  The least-squares polynomial of degree `polyorder` over `window` integer abscissae x is y -> V (V^T V)^-1 V^T y; the
    normal equations are solved in exact rational arithmetic.  taps: the weights of the fitted value at x = 0 for
    x = arange(-half, w - half)[::-1].  edge[0][r]: the weights of the fitted value at position r from the first w samples
    (positions 0 .. w - 1); edge[1][r]: position w - half + r from the last w samples.  rows: the r to compute on each side
    (default all); the others are NaN."""
    w, p = int(window), int(polyorder)
    half = w // 2
    x = [half - j for j in range(w)]
    M = [[sum(v ** (a + b) for v in x) for b in range(p + 1)] for a in range(p + 1)]
    adj, det = _int_inverse(M)
    taps = np.array([float(Fraction(sum(adj[0][a] * v ** a for a in range(p + 1)), det)) for v in x])
    # edge fit: positions 0 .. w - 1, centred on the middle sample (whole numbers: w is odd); the hat matrix does not depend on
    # the origin of the abscissae
    u = [j - half for j in range(w)]
    M = [[sum(v ** (a + b) for v in u) for b in range(p + 1)] for a in range(p + 1)]
    adj, det = _int_inverse(M)
    pw = [[v ** a for a in range(p + 1)] for v in u]
    edge = np.full((2, half, w), np.nan)
    for side in range(2):
        for r in (range(half) if rows is None else rows):
            pos = r if side == 0 else w - half + r
            g = [sum(adj[a][b] * pw[pos][b] for b in range(p + 1)) for a in range(p + 1)]
            edge[side, r] = [float(Fraction(sum(ga * va for ga, va in zip(g, pw[j])), det)) for j in range(w)]
    return taps, edge


def savgol_cases():
    """[(window, polyorder, edge rows checked per side)]"""
    out = []
    for w in (3, 5, 17, 31, 101):
        out += [(w, p, tuple(range(w // 2))) for p in range(min(15, w - 1) + 1)]
    for w in (401, 2449):
        out += [(w, p, (0, 1, w // 2 - 1)) for p in range(7)]
    return out


@functools.lru_cache(maxsize=None)
def savgol_reference_of(window, polyorder):
    rows = dict((c[:2], c[2]) for c in savgol_cases()).get((window, polyorder))
    return savgol_reference(window, polyorder, rows)


def savgol_apply(y, taps, edge):
    """scipy.signal.savgol_filter(y, w, p, mode='interp') with the given design, in numpy: interior by correlation with the
    taps, the first and last w // 2 outputs by the edge rows."""
    w = taps.size
    half = w // 2
    out = np.convolve(y, taps, mode="same")
    out[:half] = edge[0] @ y[:w]
    out[len(y) - half:] = edge[1] @ y[len(y) - w:]
    return out
